// rr_sac.hip -- Agent.choose_action of the reference's SAC trainer (Training_SAC_pytorch.py:281-285: ActorNetwork.sample_normal, :207-234)
// for a whole batch of observations in ONE launch.  The actor is Linear 11 -> 256 -> 256 -> (mu, sigma): up to its head the network of
// rr_dqn.hip, so the hidden layers ARE rr_dqn_tile.hpp's (fp32 matrix cores, transposed activations in LDS); stacked, mu and sigma are
// 2 A outputs (4 or 8), the head width the VALU loop of the Q network has.  Stock PyTorch runs a dozen small launches per call (four
// GEMMs, clamp, randn, mul / add, tanh, ...).
//
//   k_sac_act   one workgroup per CU, persistent over 64-row tiles, 256 threads.  Per tile: observations transposed into LDS ->
//               hidden_tile -> head: wavefront w computes the stacked outputs 2w and 2w + 1 (mu rows first, then sigma rows) for
//               row = lane; at A = 2 wavefronts 2 and 3 have no output and wait at the barrier -> epilogue, one lane per row:
//               csrc/rr_sac.hpp's draw (Philox4x32-10 + Box-Muller), clamp, tanh squash and log-probability.
// No atomics, nothing kept in the handle.  C-ABI and the arithmetic's specification: rr_sac_act in include/roborugby_amd.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>

#include "../../include/roborugby_amd.h"
#include "rr_dqn_shared.hpp"
#include "rr_dqn_tile.hpp"
#include "rr_sac.hpp"

namespace {

using namespace rr_tile;

constexpr int NS = 8; // stacked head outputs at most (A = 4)

struct Actor { const float *w1, *b1, *w2, *b2, *wmu, *bmu, *wsg, *bsg; };

template <int A>
__global__ __launch_bounds__(NT, 1) void k_sac_act(Actor net, const float *obs, int n, float max_action, int deterministic, uint64_t seed,
                                                   uint32_t call, float *actions, float *log_prob, float *head, float *noise) {
    __shared__ float X0[H * LDX], X1[H * LDX], S[12 * LDX], Q[NS * TM];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, half = l >> 5, c = l & 31;
    const int ntiles = n / TM;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int e = t; e < TM * IN; e += NT) {
            const int m = e / IN, ci = e - m * IN;
            S[ci * LDX + m] = obs[(size_t)(tile * TM + m) * IN + ci];
        }
        if (t < TM) S[11 * LDX + t] = 0.0f;
        __syncthreads();
        hidden_tile(net, S, X0, X1, w, half, c);
        // ---- head (2 A outputs: VALU): stacked output s < A is mu[s], s >= A is sigma[s - A]; A is even, so a wavefront's pair lies in
        // one of the two matrices.  The weights are wave-uniform.
        if (2 * w < 2 * A) {
            const int s0 = 2 * w;
            const bool is_mu = s0 < A;
            const int r0 = is_mu ? s0 : s0 - A;
            const float *wm = is_mu ? net.wmu : net.wsg, *bm = is_mu ? net.bmu : net.bsg;
            const float *wa = wm + r0 * H, *wb = wm + (r0 + 1) * H;
            float q0 = 0.0f, q1 = 0.0f;
#pragma unroll 8
            for (int k = 0; k < H; k++) {
                const float x = X1[k * LDX + l];
                q0 = fmaf(x, wa[k], q0);
                q1 = fmaf(x, wb[k], q1);
            }
            Q[s0 * TM + l] = q0 + bm[r0];
            Q[(s0 + 1) * TM + l] = q1 + bm[r0 + 1];
        }
        __syncthreads();
        // ---- epilogue: one lane per row
        if (t < TM) {
            const int row = tile * TM + t;
            float z[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
            if (!deterministic) rr::sac_draw((uint32_t)row, call, seed, z);
            float lp = 0.0f;
#pragma unroll
            for (int k = 0; k < A; k++) {
                const float mu = Q[k * TM + t], raw = Q[(A + k) * TM + t];
                const float sigma = rr::sac_sigma(raw);
                const float a = rr::sac_action(mu, sigma, z[k], max_action);
                lp += rr::sac_log_prob_term(sigma, z[k], a);
                actions[(size_t)row * A + k] = a;
                if (noise) noise[(size_t)row * A + k] = z[k];
                if (head) { head[(size_t)row * (2 * A) + k] = mu; head[(size_t)row * (2 * A) + A + k] = raw; }
            }
            if (log_prob) log_prob[row] = lp;
        }
        __syncthreads();
    }
}

} // namespace

extern "C" int rr_sac_act(rr_dqn *d, const float *const params[8], const float *obs, int32_t n, int32_t n_actions, float max_action,
                          int32_t flags, uint64_t seed, uint32_t call, float *actions, float *log_prob, float *head, float *noise,
                          void *stream) {
    if (!d || !params || !obs || !actions) return rr_dqn_fail(-1, "rr_sac_act: null argument");
    for (int k = 0; k < 8; k++) if (!params[k]) return rr_dqn_fail(-1, "rr_sac_act: null parameter pointer");
    if (n <= 0 || n % TM) return rr_dqn_fail(-1, "rr_sac_act: the number of observations must be a positive multiple of 64");
    if (n_actions != 2 && n_actions != 4) return rr_dqn_fail(-1, "rr_sac_act: n_actions must be 2 or 4");
    if (!std::isfinite(max_action) || !(max_action > 0.0f)) return rr_dqn_fail(-1, "rr_sac_act: max_action must be finite and > 0");
    if (flags & ~RR_SAC_DETERMINISTIC) return rr_dqn_fail(-1, "rr_sac_act: unknown flag bits");
    int prev = -1;
    const bool sw = hipGetDevice(&prev) == hipSuccess && prev != d->device && hipSetDevice(d->device) == hipSuccess;
    const Actor net = { params[0], params[1], params[2], params[3], params[4], params[5], params[6], params[7] };
    const int ntiles = n / TM, nwg = ntiles < d->nwg ? ntiles : d->nwg, det = flags & RR_SAC_DETERMINISTIC ? 1 : 0;
    if (n_actions == 2)
        hipLaunchKernelGGL(k_sac_act<2>, dim3(nwg), dim3(NT), 0, (hipStream_t)stream, net, obs, (int)n, max_action, det, seed, call, actions,
                           log_prob, head, noise);
    else
        hipLaunchKernelGGL(k_sac_act<4>, dim3(nwg), dim3(NT), 0, (hipStream_t)stream, net, obs, (int)n, max_action, det, seed, call, actions,
                           log_prob, head, noise);
    const hipError_t e = hipGetLastError();
    if (sw) (void)hipSetDevice(prev);
    if (e != hipSuccess) return rr_dqn_fail(-2, hipGetErrorString(e));
    return 0;
}
