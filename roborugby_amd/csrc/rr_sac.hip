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
//
// ... and three of the four backward passes of Agent.learn (:344-383): the value net and the two critics are each a Linear K -> 256 ->
// 256 -> 1 MLP regressed onto a constant target vector with 0.5 * mse_loss (K = 11, 11 + A), which needs no autograd:
//
//   k_sac_grads   rr_dqn.hip's k_dqn_fwd_bwd with a scalar head and no target net: 256 threads, one workgroup per CU, 64-row tiles, the
//               activations transposed in LDS at row stride 65, the dW2 accumulators resident in registers over a work item's tiles
//               (256 per lane), dW1 / dWo / db* per-thread VALU accumulators.  A workgroup's accumulators belong to one net at a time,
//               so the work item is (net, chunk): with G workgroups a net has C = max(1, G / 3) chunks, the items are numbered net-major
//               and dealt round-robin (G < 3: a workgroup takes several, one after the other, and zeroes its accumulators in between);
//               item (net, c) takes the tiles c, c + C, ... and writes ONE partial into slot (net, c); a chunk without a tile writes
//               nothing.  min(G, 3 C) workgroups are launched: one that would have no item (G = 7: six items) is not, one whose chunk has
//               no tile (B = 4,096 on 256 CUs: 63 of 255) exits at once.  Per tile: inputs [s] or [s, a] -> hidden_tile<K> -> the single output f (single_head) -> d = (f - y) / B,
//               loss += (f - y)^2 -> fc3 backward (VALU; relu' = h > 0 as torch has it) -> dW2 += dh2^T h1 (MFMA) -> dh1 = (dh2 W2) *
//               relu' (MFMA) -> dW1, db1 (VALU).
//   k_sac_grads_reduce   sums a net's min(C, B / 64) slots in chunk order (fp32), scatters the sums into the caller's six tensors per net
//               and writes loss_j = 0.5 * sum (f - y)^2 / B.
// THE CONTRACT: for net j with input x and target y, f = the fp32 forward (hidden_tile's layers, then an fp32 dot plus the bias); the
// output gradient of a row is d = (f - y) / B (one subtraction, one multiplication by fl(1 / B)); loss_j = 0.5 * mean (f - y)^2, so
// value_loss = loss[0] and critic_loss = loss[1] + loss[2]; every sum is fp32, in no particular order inside a tile.  No atomics; every
// element of every output is written by every call; the handle keeps nothing but the partials scratch (allocated by the first call,
// grown by a call that needs more slots).  Bit-identical from call to call for a given (B, G); NOT across grid sizes (RR_DQN_WGS): the
// partial sums regroup.  Inputs must be finite: a NaN row (rr_sac_targets writes one for a ring row outside the rings) makes the
// gradients NaN, and nothing here handles it.  C-ABI: rr_sac_grads in include/roborugby_amd.h.
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
template <class NetT>
__device__ __forceinline__ void single_head(const NetT &net, const float *X1, float *part, float *out, int t, int w, int l) {
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

// ---- rr_sac_grads
// (a type of its own: hidden_tile and single_head are instantiated apart from k_sac_targets' -- the optimiser specialises a shared
// instantiation for all of its callers together, and k_sac_targets keeps the code it had)
struct GradNet : Mlp1 {};
struct GradsArgs {
    GradNet value, critic_1, critic_2;
    const float *state, *action, *value_target, *q_hat;
    int batch, chunks, slots;  // chunks per net (C); slots per net in `partials` = min(C, tiles)
    float *partials;
};
struct GradsOut { float *grad[rr::SAC_GRADS_NETS][6]; float *loss; };

// one work item: the tiles chunk, chunk + chunks, ... of one net with K inputs (K odd: the pad row of S is row K), regressed onto
// `target`; the partial gradient goes to `out` (a slot: rr::sac_grads_layout(K, H)).  Ends behind a barrier: the next item may reuse LDS.
template <int K>
__device__ __forceinline__ void grads_item(const GradNet &net, const float *state, const float *action, const float *target, int batch, int chunk,
                                           int chunks, float *out, float *X0, float *X1, float *S, float *P, float *QV, float *DQ, float *RED) {
    static_assert(K % 2 == 1 && K >= IN && K <= 15, "S holds K + 1 <= 16 rows");
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // gradient accumulators that stay in registers over all of this item's tiles
    f16v dw2[16]; // [it (i-tile 2w+it)][jt]: dW2[i][j], i = out feature of fc2, j = in feature
#pragma unroll
    for (int q = 0; q < 16; q++) dw2[q] = (f16v)0.0f;
    float dw1[K];
#pragma unroll
    for (int q = 0; q < K; q++) dw1[q] = 0.0f;
    float dwo = 0.0f, db1 = 0.0f, db2 = 0.0f, dbo = 0.0f, loss = 0.0f;
    const float wo_t = net.wo[threadIdx.x];
    const float inv_b = 1.0f / (float)batch;
    const int ntiles = batch / TM;
    for (int tile = chunk; tile < ntiles; tile += chunks) {
        // (the lane index is opaque per tile: hoisted out of this loop, a tile's address arithmetic does not fit next to the 256
        // accumulators -- it is cheap to redo and costly to spill)
        int l = lane;
        asm volatile("" : "+v"(l));
        const int t = w * 64 + l, half = l >> 5, c = l & 31;
        // ---- the tile's inputs transposed into LDS: the state, for a critic the action behind it, the pad row
        for (int e = t; e < TM * IN; e += NT) {
            const int m = e / IN, ci = e - m * IN;
            S[ci * LDX + m] = state[(size_t)(tile * TM + m) * IN + ci];
        }
        if (K > IN) {
            constexpr int A = K > IN ? K - IN : 1;
            for (int e = t; e < TM * A; e += NT) {
                const int m = e / A, ci = e - m * A;
                S[(IN + ci) * LDX + m] = action[(size_t)tile * TM * A + e];
            }
        }
        if (t < TM) S[K * LDX + t] = 0.0f;
        __syncthreads();
        // ---- forward: h1 -> X0, h2 -> X1, f -> QV; the output gradient d = (f - y) / B
        hidden_tile<K>(net, S, X0, X1, w, half, c);
        single_head(net, X1, P, QV, t, w, l);
        if (t < TM) {
            const float diff = QV[t] - target[tile * TM + t];
            DQ[t] = diff * inv_b;
            loss += diff * diff;
        }
        __syncthreads();
        // ---- fc3 backward (one output): thread t owns hidden unit n = t.  dWo[n] += d h2, then X1 <- dh2 = d Wo[n] relu'(h2)
        {
            float *row = &X1[t * LDX];
#pragma unroll 4
            for (int m = 0; m < TM; m++) {
                const float d = DQ[m];   // wave-uniform: LDS broadcast
                const float h = row[m];
                dwo += d * h;
                const float gr = h > 0.0f ? d * wo_t : 0.0f;
                row[m] = gr;
                db2 += gr;
            }
            if (t == 0) {
#pragma unroll 4
                for (int m = 0; m < TM; m++) dbo += DQ[m];
            }
        }
        __syncthreads();
        // ---- dW2[i][j] += sum_m dh2[m][i] h1[m][j]: reduction over the tile's 64 samples, two per MFMA
#pragma unroll 2
        for (int p = 0; p < TM / 2; p++) {
            const int mm = 2 * p + half;
            const float a0 = X1[((2 * w) * 32 + c) * LDX + mm], a1 = X1[((2 * w + 1) * 32 + c) * LDX + mm];
#pragma unroll
            for (int jt = 0; jt < 8; jt++) {
                const float b = X0[(jt * 32 + c) * LDX + mm];
                dw2[jt] = mfma(a0, b, dw2[jt]);
                dw2[8 + jt] = mfma(a1, b, dw2[8 + jt]);
            }
        }
        // ---- dh1[m][k] = sum_n dh2[m][n] W2[n][k] (then * relu'(h1)): output k-tiles {2w, 2w+1} x m-tiles {0, 1}
        {
            f16v acc[4];
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] = (f16v)0.0f;
            const float *w2c0 = net.w2 + (2 * w) * 32 + c, *w2c1 = net.w2 + (2 * w + 1) * 32 + c;
#pragma unroll 4
            for (int np = 0; np < H / 2; np++) {
                const int n = 2 * np + half;
                const float a0 = X1[n * LDX + c], a1 = X1[n * LDX + 32 + c];
                const float b0 = w2c0[n * H], b1 = w2c1[n * H];
                acc[0] = mfma(a0, b0, acc[0]);
                acc[1] = mfma(a1, b0, acc[1]);
                acc[2] = mfma(a0, b1, acc[2]);
                acc[3] = mfma(a1, b1, acc[3]);
            }
            __syncthreads(); // every wavefront has read h1 (X0) for dW2: it can be overwritten with dh1 now
#pragma unroll
            for (int kt = 0; kt < 2; kt++) {
                const int k = (2 * w + kt) * 32 + c;
#pragma unroll
                for (int mt = 0; mt < 2; mt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        float *px = &X0[k * LDX + mt * 32 + acc_row(r, half)];
                        *px = *px > 0.0f ? acc[kt * 2 + mt][r] : 0.0f;
                    }
            }
        }
        __syncthreads();
        // ---- fc1 backward: thread t owns hidden unit k = t: db1, dW1[k][:] += dh1[m][k] x[m][:]
        {
            const float *row = &X0[t * LDX];
#pragma unroll 4
            for (int m = 0; m < TM; m++) {
                const float gr = row[m];
                db1 += gr;
#pragma unroll
                for (int ci = 0; ci < K; ci++) dw1[ci] = fmaf(gr, S[ci * LDX + m], dw1[ci]);
            }
        }
        __syncthreads();
    }
    // ---- this item's partial gradient
    int l = lane;
    asm volatile("" : "+v"(l));  // (... nor do the 256 store addresses, computed ahead of the tile loop)
    const int t = w * 64 + l, half = l >> 5, c = l & 31;
    const rr::SacGradsLayout L = rr::sac_grads_layout(K, H);
#pragma unroll
    for (int it = 0; it < 2; it++)
#pragma unroll
        for (int jt = 0; jt < 8; jt++)
#pragma unroll
            for (int r = 0; r < 16; r++)
                out[L.w2 + ((2 * w + it) * 32 + acc_row(r, half)) * H + jt * 32 + c] = dw2[it * 8 + jt][r];
#pragma unroll
    for (int ci = 0; ci < K; ci++) out[L.w1 + t * K + ci] = dw1[ci];
    out[L.wo + t] = dwo;
    out[L.b1 + t] = db1;
    out[L.b2 + t] = db2;
    if (t < TM) RED[t] = loss;
    __syncthreads();
    if (t == 0) {
        out[L.bo] = dbo;
        float s = 0.0f;
        for (int q = 0; q < TM; q++) s += RED[q];
        out[L.loss] = s;
    }
    __syncthreads();
}

template <int A>
__global__ __launch_bounds__(NT, 1) void k_sac_grads(GradsArgs g) {
    __shared__ float X0[H * LDX], X1[H * LDX], S[16 * LDX], P[4 * TM], QV[TM], DQ[TM], RED[TM];
    const int C = g.chunks, G = (int)gridDim.x, items = rr::SAC_GRADS_NETS * C;
    const int live = g.slots;  // chunks of a net that have a tile; the others have no slot and write nothing
    // items 0 .. C-1 are the value net's, C .. 3C-1 the critics', dealt round-robin: a workgroup's value items first (one loop per
    // input width: each keeps one set of accumulators)
    for (int item = (int)blockIdx.x; item < C; item += G) {
        if (item >= live) break;
        grads_item<IN>(g.value, g.state, nullptr, g.value_target, g.batch, item, C, g.partials + (size_t)item * rr::SAC_GRADS_STRIDE, X0, X1, S, P,
                       QV, DQ, RED);
    }
    const int first = C + (((int)blockIdx.x - C) % G + G) % G;  // this workgroup's first item >= C
    for (int item = first; item < items; item += G) {
        const int net = item / C, chunk = item - net * C;
        if (chunk >= live) continue;
        grads_item<IN + A>(net == 1 ? g.critic_1 : g.critic_2, g.state, g.action, g.q_hat, g.batch, chunk, C, g.partials +
                           (size_t)(net * live + chunk) * rr::SAC_GRADS_STRIDE, X0, X1, S, P, QV, DQ, RED);
    }
}

// element i of net blockIdx.y's slot layout: the sum of its `slots` partials in chunk order -> the caller's tensor (torch.nn.Linear
// layouts), or the loss
__global__ __launch_bounds__(256) void k_sac_grads_reduce(const float *partials, int slots, int n_actions, int batch, GradsOut o) {
    const int net = (int)blockIdx.y, i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const rr::SacGradsLayout L = rr::sac_grads_layout(net == 0 ? IN : IN + n_actions, H);
    if (i >= L.count) return;
    const float *p = partials + (size_t)net * slots * rr::SAC_GRADS_STRIDE + i;
    float s = 0.0f;
#pragma unroll 8
    for (int ch = 0; ch < slots; ch++) s += p[(size_t)ch * rr::SAC_GRADS_STRIDE];  // (the loads do not wait for the sum: only the adds are a chain)
    float *const *gr = o.grad[net];
    if (i < L.w1) gr[2][i - L.w2] = s;
    else if (i < L.wo) gr[0][i - L.w1] = s;
    else if (i < L.b1) gr[4][i - L.wo] = s;
    else if (i < L.b2) gr[1][i - L.b1] = s;
    else if (i < L.bo) gr[3][i - L.b2] = s;
    else if (i < L.loss) gr[5][0] = s;
    else o.loss[net] = 0.5f * s / (float)batch;
}

} // namespace

extern "C" int rr_sac_grads(rr_dqn *d, const rr_sac_grads_args *a, void *stream) {
    if (!d || !a) return rr_dqn_fail(-1, "rr_sac_grads: null argument");
    if (a->struct_size != (int32_t)sizeof(rr_sac_grads_args)) return rr_dqn_fail(-1, "rr_sac_grads: struct_size does not match this library");
    for (int k = 0; k < 6; k++) {
        if (!a->value[k] || !a->critic_1[k] || !a->critic_2[k]) return rr_dqn_fail(-1, "rr_sac_grads: null parameter pointer");
        if (!a->grad_value[k] || !a->grad_critic_1[k] || !a->grad_critic_2[k]) return rr_dqn_fail(-1, "rr_sac_grads: null gradient pointer");
    }
    if (!a->state || !a->action || !a->value_target || !a->q_hat) return rr_dqn_fail(-1, "rr_sac_grads: state, action, value_target and q_hat are required");
    if (!a->loss) return rr_dqn_fail(-1, "rr_sac_grads: loss is required");
    if (a->batch <= 0 || a->batch % TM) return rr_dqn_fail(-1, "rr_sac_grads: batch must be a positive multiple of 64");
    if (a->n_actions != 2 && a->n_actions != 4) return rr_dqn_fail(-1, "rr_sac_grads: n_actions must be 2 or 4");
    if (a->flags) return rr_dqn_fail(-1, "rr_sac_grads: flags must be 0");
    const auto mlp = [](const float *const p[6]) { return GradNet{ { p[0], p[1], p[2], p[3], p[4], p[5] } }; };
    GradsArgs g;
    g.value = mlp(a->value); g.critic_1 = mlp(a->critic_1); g.critic_2 = mlp(a->critic_2);
    g.state = a->state; g.action = a->action; g.value_target = a->value_target; g.q_hat = a->q_hat;
    g.batch = a->batch;
    g.chunks = rr::sac_grads_chunks(d->nwg);
    g.slots = rr::sac_grads_slots(g.chunks, a->batch / TM);
    GradsOut o;
    for (int k = 0; k < 6; k++) { o.grad[0][k] = a->grad_value[k]; o.grad[1][k] = a->grad_critic_1[k]; o.grad[2][k] = a->grad_critic_2[k]; }
    o.loss = a->loss;
    int prev = -1;
    const bool sw = hipGetDevice(&prev) == hipSuccess && prev != d->device && hipSetDevice(d->device) == hipSuccess;
    const size_t need = (size_t)rr::SAC_GRADS_NETS * (size_t)g.slots;
    if (need > d->sac_cap) {  // (hipFree waits for the launches that still read the old scratch)
        if (d->sac_partials) (void)hipFree(d->sac_partials);
        d->sac_partials = nullptr; d->sac_cap = 0;
        if (hipMalloc((void **)&d->sac_partials, sizeof(float) * rr::SAC_GRADS_STRIDE * need) != hipSuccess) {
            d->sac_partials = nullptr;
            if (sw) (void)hipSetDevice(prev);
            return rr_dqn_fail(-3, "rr_sac_grads: out of device memory");
        }
        d->sac_cap = need;
    }
    g.partials = d->sac_partials;
    const int items = rr::SAC_GRADS_NETS * g.chunks, nwg = items < d->nwg ? items : d->nwg;
    if (a->n_actions == 2)
        hipLaunchKernelGGL(k_sac_grads<2>, dim3(nwg), dim3(NT), 0, (hipStream_t)stream, g);
    else
        hipLaunchKernelGGL(k_sac_grads<4>, dim3(nwg), dim3(NT), 0, (hipStream_t)stream, g);
    const int count = rr::sac_grads_layout(IN + 4, H).count;
    hipLaunchKernelGGL(k_sac_grads_reduce, dim3((count + 255) / 256, rr::SAC_GRADS_NETS), dim3(256), 0, (hipStream_t)stream,
                       (const float *)d->sac_partials, g.slots, (int)a->n_actions, (int)a->batch, o);
    const hipError_t e = hipGetLastError();
    if (sw) (void)hipSetDevice(prev);
    if (e != hipSuccess) return rr_dqn_fail(-2, hipGetErrorString(e));
    return 0;
}

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
