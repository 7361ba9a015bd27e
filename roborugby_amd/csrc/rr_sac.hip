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
//
// ... and the no-grad half of Agent.learn (:344-383) for a batch gathered out of the replay rings, in ONE launch as well:
//
//   k_sac_targets   the same workgroups, persistent over work items (role, 64-row tile).  Role 0: the rows' states gathered into LDS ->
//               the actor as above (the draw on stream word 0x5A7A, or fed in) -> the sampled action appended to the input tile ->
//               critic_1, critic_2 (hidden_tile with K = 11 + A; the single output: each wavefront sums 64 of the 256 products per
//               row, one lane per row adds the four partial sums in order and the bias) -> value_target = min(q1, q2) - log_prob.
//               Role 1: the rows' next states -> the target value net -> q_hat = scale r + gamma (done ? 0 : v).  The two roles share
//               nothing, so the items 0 .. tiles-1 are role 0 and tiles .. 2 tiles-1 role 1: at 4,096 rows (64 tiles) twice as many
//               CUs work.  X0 / X1 are reused by the nets one after another.  A ring row outside [0, mem_rows) is computed as a row of
//               zeros and written as NaN.
// No atomics, nothing kept in the handle.  C-ABI and the arithmetic's specification: rr_sac_act / rr_sac_targets in
// include/roborugby_amd.h.
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

// ---- rr_sac_targets
struct Mlp1 { const float *w1, *b1, *w2, *b2, *wo, *bo; };  // two hidden layers and a single output (critic: q, value net: v)

struct TargetsArgs {
    Actor actor;
    Mlp1 critic_1, critic_2, target_value;
    const float *state_memory, *new_state_memory, *action_memory, *reward_memory;
    const uint8_t *terminal_memory;
    long long mem_rows;
    const long long *batch_index;
    const float *noise;
    float max_action, gamma, reward_scale;
    uint64_t seed;
    uint32_t call;
    int batch;
    float *value_target, *q_hat, *state, *action, *policy_action, *log_prob, *head, *noise_out, *q1, *q2, *v_next;
};

// ring rows of the tile's 64 batch rows (-1: outside the rings, never an address), then the rows' 11 observations of `ring` transposed
// into S (zeros for such a row; the pad row 11 = 0); `out`, if given, receives the gathered rows (NaN for such a row).  Ends behind a
// barrier.
__device__ __forceinline__ void gather_tile(const TargetsArgs &g, const float *ring, float *out, int tile, int t, long long *ridx, float *S) {
    if (t < TM) {
        const int row = tile * TM + t;
        const long long i = g.batch_index ? g.batch_index[row] : (long long)row;
        ridx[t] = rr::sac_ring_row_ok(i, g.mem_rows) ? i : -1;
    }
    __syncthreads();
    for (int e = t; e < TM * IN; e += NT) {
        const int m = e / IN, ci = e - m * IN;
        const long long i = ridx[m];
        const float v = i >= 0 ? ring[(size_t)i * IN + ci] : 0.0f;
        S[ci * LDX + m] = v;
        if (out) out[(size_t)(tile * TM + m) * IN + ci] = i >= 0 ? v : NAN;
    }
    if (t < TM) S[IN * LDX + t] = 0.0f;
    __syncthreads();
}

// the single output of a net whose second hidden layer is in X1: wavefront w sums the products k = 64 w .. 64 w + 63 of row = lane in
// order, lane `row` of wavefront 0 adds the four partial sums in order and the bias -> out[row] (LDS).  Ends behind a barrier.
__device__ __forceinline__ void single_head(const Mlp1 &net, const float *X1, float *part, float *out, int t, int w, int l) {
    const float *wo = net.wo + w * (H / 4);
    float q = 0.0f;
#pragma unroll 8
    for (int k = 0; k < H / 4; k++) q = fmaf(X1[(w * (H / 4) + k) * LDX + l], wo[k], q);
    part[w * TM + l] = q;
    __syncthreads();
    if (t < TM) out[t] = ((part[t] + part[TM + t]) + part[2 * TM + t]) + part[3 * TM + t] + net.bo[0];
    __syncthreads();
}

template <int A>
__global__ __launch_bounds__(NT, 1) void k_sac_targets(TargetsArgs g) {
    __shared__ float X0[H * LDX], X1[H * LDX], S[16 * LDX], Q[NS * TM], P[4 * TM], QV[2 * TM], LP[TM];
    __shared__ long long ridx[TM];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, half = l >> 5, c = l & 31;
    const int ntiles = g.batch / TM;
    // work items 0 .. ntiles-1 are role 0, ntiles .. 2 ntiles-1 role 1, dealt round-robin: a workgroup's role 0 items first (one loop
    // per role: each keeps only its own pointers in scalar registers)
    {
        // ---- role 0: actor -> critic_1, critic_2 -> value_target
        for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
            gather_tile(g, g.state_memory, g.state, tile, t, ridx, S);
            if (g.action)
                for (int e = t; e < TM * A; e += NT) {
                    const int m = e / A;
                    const long long i = ridx[m];
                    g.action[(size_t)tile * TM * A + e] = i >= 0 ? g.action_memory[(size_t)i * A + (e - m * A)] : NAN;
                }
            hidden_tile(g.actor, S, X0, X1, w, half, c);
            if (2 * w < 2 * A) {  // k_sac_act's head
                const int s0 = 2 * w;
                const bool is_mu = s0 < A;
                const int r0 = is_mu ? s0 : s0 - A;
                const float *wm = is_mu ? g.actor.wmu : g.actor.wsg, *bm = is_mu ? g.actor.bmu : g.actor.bsg;
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
            // ---- the sample, one lane per row: its action becomes the critics' inputs 11 .. 11 + A - 1 (the pad row 11 + A = 0)
            if (t < TM) {
                const int row = tile * TM + t;
                const bool ok = ridx[t] >= 0;
                float z[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                if (g.noise) {
#pragma unroll
                    for (int k = 0; k < A; k++) z[k] = g.noise[(size_t)row * A + k];
                } else {
                    rr::sac_draw((uint32_t)row, g.call, g.seed, z, rr::SAC_TARGETS_STREAM);
                }
                float lp = 0.0f;
#pragma unroll
                for (int k = 0; k < A; k++) {
                    const float mu = Q[k * TM + t], raw = Q[(A + k) * TM + t];
                    const float sigma = rr::sac_sigma(raw);
                    const float a = rr::sac_action(mu, sigma, z[k], g.max_action);
                    lp += rr::sac_log_prob_term(sigma, z[k], a);
                    S[(IN + k) * LDX + t] = a;
                    if (g.policy_action) g.policy_action[(size_t)row * A + k] = ok ? a : NAN;
                    if (g.noise_out) g.noise_out[(size_t)row * A + k] = ok ? z[k] : NAN;
                    if (g.head) { g.head[(size_t)row * (2 * A) + k] = ok ? mu : NAN; g.head[(size_t)row * (2 * A) + A + k] = ok ? raw : NAN; }
                }
                S[(IN + A) * LDX + t] = 0.0f;
                LP[t] = lp;
                if (g.log_prob) g.log_prob[row] = ok ? lp : NAN;
            }
            __syncthreads();
            hidden_tile<IN + A>(g.critic_1, S, X0, X1, w, half, c);
            single_head(g.critic_1, X1, P, QV, t, w, l);
            hidden_tile<IN + A>(g.critic_2, S, X0, X1, w, half, c);
            single_head(g.critic_2, X1, P, QV + TM, t, w, l);
            if (t < TM) {
                const int row = tile * TM + t;
                const bool ok = ridx[t] >= 0;
                const float q1 = QV[t], q2 = QV[TM + t];
                g.value_target[row] = ok ? rr::sac_value_target(q1, q2, LP[t]) : NAN;
                if (g.q1) g.q1[row] = ok ? q1 : NAN;
                if (g.q2) g.q2[row] = ok ? q2 : NAN;
            }
            __syncthreads();
        }
        // ---- role 1: target value net on the next states -> q_hat
        const int G = (int)gridDim.x, first = (((int)blockIdx.x - ntiles) % G + G) % G;  // the first item >= ntiles of this workgroup, less ntiles
        for (int tile = first; tile < ntiles; tile += G) {
            gather_tile(g, g.new_state_memory, nullptr, tile, t, ridx, S);
            hidden_tile(g.target_value, S, X0, X1, w, half, c);
            single_head(g.target_value, X1, P, QV, t, w, l);
            if (t < TM) {
                const int row = tile * TM + t;
                const long long i = ridx[t];
                const float v = QV[t];
                g.q_hat[row] = i >= 0 ? rr::sac_q_hat(g.reward_scale, g.reward_memory[i], g.gamma, g.terminal_memory[i] != 0, v) : NAN;
                if (g.v_next) g.v_next[row] = i >= 0 ? v : NAN;
            }
            __syncthreads();
        }
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

extern "C" int rr_sac_targets(rr_dqn *d, const rr_sac_targets_args *a, void *stream) {
    if (!d || !a) return rr_dqn_fail(-1, "rr_sac_targets: null argument");
    if (a->struct_size != (int32_t)sizeof(rr_sac_targets_args)) return rr_dqn_fail(-1, "rr_sac_targets: struct_size does not match this library");
    for (int k = 0; k < 8; k++) if (!a->actor[k]) return rr_dqn_fail(-1, "rr_sac_targets: null parameter pointer");
    for (int k = 0; k < 6; k++)
        if (!a->critic_1[k] || !a->critic_2[k] || !a->target_value[k]) return rr_dqn_fail(-1, "rr_sac_targets: null parameter pointer");
    if (!a->state_memory || !a->new_state_memory || !a->action_memory || !a->reward_memory || !a->terminal_memory)
        return rr_dqn_fail(-1, "rr_sac_targets: null replay ring");
    if (!a->value_target || !a->q_hat) return rr_dqn_fail(-1, "rr_sac_targets: value_target and q_hat are required");
    if (a->batch <= 0 || a->batch % TM) return rr_dqn_fail(-1, "rr_sac_targets: batch must be a positive multiple of 64");
    if (a->n_actions != 2 && a->n_actions != 4) return rr_dqn_fail(-1, "rr_sac_targets: n_actions must be 2 or 4");
    if (a->mem_rows < 1) return rr_dqn_fail(-1, "rr_sac_targets: mem_rows must be >= 1");
    if (!a->batch_index && a->mem_rows < a->batch) return rr_dqn_fail(-1, "rr_sac_targets: without batch_index the rings must hold batch rows");
    if (!std::isfinite(a->max_action) || !(a->max_action > 0.0f)) return rr_dqn_fail(-1, "rr_sac_targets: max_action must be finite and > 0");
    if (!std::isfinite(a->gamma) || !std::isfinite(a->reward_scale)) return rr_dqn_fail(-1, "rr_sac_targets: gamma and reward_scale must be finite");
    if (a->flags) return rr_dqn_fail(-1, "rr_sac_targets: flags must be 0");
    const auto mlp = [](const float *const p[6]) { return Mlp1{ p[0], p[1], p[2], p[3], p[4], p[5] }; };
    TargetsArgs g;
    g.actor = { a->actor[0], a->actor[1], a->actor[2], a->actor[3], a->actor[4], a->actor[5], a->actor[6], a->actor[7] };
    g.critic_1 = mlp(a->critic_1); g.critic_2 = mlp(a->critic_2); g.target_value = mlp(a->target_value);
    g.state_memory = a->state_memory; g.new_state_memory = a->new_state_memory; g.action_memory = a->action_memory;
    g.reward_memory = a->reward_memory; g.terminal_memory = a->terminal_memory;
    g.mem_rows = a->mem_rows; g.batch_index = (const long long *)a->batch_index; g.noise = a->noise;
    g.max_action = a->max_action; g.gamma = a->gamma; g.reward_scale = a->reward_scale;
    g.seed = a->seed; g.call = a->call; g.batch = a->batch;
    g.value_target = a->value_target; g.q_hat = a->q_hat; g.state = a->state; g.action = a->action;
    g.policy_action = a->policy_action; g.log_prob = a->log_prob; g.head = a->head; g.noise_out = a->noise_out;
    g.q1 = a->q1; g.q2 = a->q2; g.v_next = a->v_next;
    int prev = -1;
    const bool sw = hipGetDevice(&prev) == hipSuccess && prev != d->device && hipSetDevice(d->device) == hipSuccess;
    const int items = 2 * (a->batch / TM), nwg = items < d->nwg ? items : d->nwg;
    if (a->n_actions == 2)
        hipLaunchKernelGGL(k_sac_targets<2>, dim3(nwg), dim3(NT), 0, (hipStream_t)stream, g);
    else
        hipLaunchKernelGGL(k_sac_targets<4>, dim3(nwg), dim3(NT), 0, (hipStream_t)stream, g);
    const hipError_t e = hipGetLastError();
    if (sw) (void)hipSetDevice(prev);
    if (e != hipSuccess) return rr_dqn_fail(-2, hipGetErrorString(e));
    return 0;
}
