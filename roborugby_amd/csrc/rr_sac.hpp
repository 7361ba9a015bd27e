// rr_sac.hpp -- the per-row arithmetic of rr_sac_act's and rr_sac_targets' epilogues (include/roborugby_amd.h is the specification): the
// standard normal draws of a row, the clamp of sigma, the squashed action and a component's share of the log-probability; the gather's
// bounds rule and the two closing formulas of the learn targets; rr_sac_grads' work items and the layout of its partial slots.  Plain
// C++ as well as HIP: tests/emu/rr_sac_emu.cpp and tests/emu/rr_sac_targets_emu.cpp compile the per-row functions with g++ and hold them
// to tests/sac_ref.py / tests/sac_targets_ref.py without a GPU.
#pragma once
#include <math.h>
#include "rr_dqn_shared.hpp"

namespace rr {

constexpr uint32_t SAC_STREAM = 0x5AC7u;  // counter word 2 of the draws (rr_dqn_act / rr_cnn_act: 0x0AC7, rr_frames_sample: 0x5A3E)
constexpr uint32_t SAC_TARGETS_STREAM = 0x5A7Au;  // ... of rr_sac_targets' draws: one (seed, call) never correlates acting and learning
constexpr float SAC_SIGMA_MIN = 1e-6f, SAC_SIGMA_MAX = 1.0f;  // ActorNetwork.forward: clamp(sigma, reparam_noise, 1)
constexpr float SAC_LOG_EPS = 1e-6f;                          // ... sample_normal: log(1 - a^2 + reparam_noise)
constexpr float SAC_TWO_PI = 6.2831853071795865f, SAC_HALF_LOG_TWO_PI = 0.91893853320467274f;
constexpr float SAC_2M24 = 5.9604644775390625e-8f;

// two 32-bit words -> u1 in (0, 1], u2 in [0, 1): multiples of 2^-24, exact in fp32
RR_DQN_HD void sac_uniforms(uint32_t wa, uint32_t wb, float &u1, float &u2) {
    u1 = (float)((wa >> 8) + 1u) * SAC_2M24;
    u2 = (float)(wb >> 8) * SAC_2M24;
}
// Box-Muller: two independent standard normals from (u1, u2)
RR_DQN_HD void sac_box_muller(float u1, float u2, float &z0, float &z1) {
    const float r = sqrtf(-2.0f * logf(u1)), a = SAC_TWO_PI * u2;
    z0 = r * cosf(a);
    z1 = r * sinf(a);
}
// the four draws of row `row` in call `call`: Philox4x32-10, counter (row, call, stream, 0), key = seed (low word, high word)
RR_DQN_HD void sac_draw(uint32_t row, uint32_t call, uint64_t seed, float z[4], uint32_t stream = SAC_STREAM) {
    uint32_t w[4] = { row, call, stream, 0u };
    philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
    float u1, u2;
    sac_uniforms(w[0], w[1], u1, u2);
    sac_box_muller(u1, u2, z[0], z[1]);
    sac_uniforms(w[2], w[3], u1, u2);
    sac_box_muller(u1, u2, z[2], z[3]);
}
// torch.clamp(raw, 1e-6, 1): a NaN stays a NaN
RR_DQN_HD float sac_sigma(float raw) { return raw < SAC_SIGMA_MIN ? SAC_SIGMA_MIN : (raw > SAC_SIGMA_MAX ? SAC_SIGMA_MAX : raw); }
RR_DQN_HD float sac_action(float mu, float sigma, float z, float max_action) { return max_action * tanhf(mu + sigma * z); }
// Normal(mu, sigma).log_prob(mu + sigma z) - log(1 - a^2 + 1e-6) of one component (a: the SCALED action, as the reference has it)
RR_DQN_HD float sac_log_prob_term(float sigma, float z, float a) {
    return -0.5f * z * z - logf(sigma) - SAC_HALF_LOG_TWO_PI - logf(1.0f - a * a + SAC_LOG_EPS);
}

// ---- rr_sac_targets
// the gather's bounds rule: ring row i may be used as an address
RR_DQN_HD bool sac_ring_row_ok(int64_t i, int64_t mem_rows) { return i >= 0 && i < mem_rows; }
// value_target = min(Q1, Q2) - log pi: one subtraction of the fp32 numbers the windows report
RR_DQN_HD float sac_value_target(float q1, float q2, float log_prob) { return fminf(q1, q2) - log_prob; }
// q_hat = reward_scale r + gamma (done ? 0 : V_target(s')): two rounded products and their rounded sum (no contraction)
RR_DQN_HD float sac_q_hat(float reward_scale, float r, float gamma, bool done, float v_next) {
    const float a = reward_scale * r, b = gamma * (done ? 0.0f : v_next);
    return a + b;
}

// ---- rr_sac_grads
// work items and partial slots: G workgroups give every net C = max(1, G / 3) chunks; chunk c of a net takes the 64-row tiles c, c + C,
// ...; of a net's chunks only the first min(C, tiles) have a tile, and only those have a slot in the scratch (slot = net * slots + c)
constexpr int SAC_GRADS_NETS = 3;  // value, critic_1, critic_2
RR_DQN_HD int sac_grads_chunks(int nwg) { return nwg / SAC_GRADS_NETS > 1 ? nwg / SAC_GRADS_NETS : 1; }
RR_DQN_HD int sac_grads_slots(int chunks, int tiles) { return chunks < tiles ? chunks : tiles; }
// a slot (floats) of a net with K inputs and hidden width W: dW2 [W, W], dW1 [W, K], dWo [W], db1 [W], db2 [W], dbo, sum (f - y)^2
struct SacGradsLayout { int w2, w1, wo, b1, b2, bo, loss, count; };
RR_DQN_HD SacGradsLayout sac_grads_layout(int K, int W) {
    SacGradsLayout s;
    s.w2 = 0; s.w1 = s.w2 + W * W; s.wo = s.w1 + W * K; s.b1 = s.wo + W; s.b2 = s.b1 + W; s.bo = s.b2 + W; s.loss = s.bo + 1; s.count = s.loss + 1;
    return s;
}
// the stride of a slot: the widest net's (K = 11 + 4) count, rounded up to 64 floats
constexpr int SAC_GRADS_STRIDE = ((256 * 256 + 256 * 15 + 3 * 256 + 2 + 63) / 64) * 64;

} // namespace rr
