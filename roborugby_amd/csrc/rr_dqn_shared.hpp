// rr_dqn_shared.hpp -- what the translation units behind the rr_dqn handle share (rr_dqn.hip: the lidar agent's fused kernels;
// rr_cnn.hip: the pixel agent's forward; rr_sac.hip: the SAC actor's, whose draws take the Philox rounds below): the handle itself, the error string's setter and the epsilon-greedy draw, so that
// rr_dqn_act and rr_cnn_act explore the same rows with the same actions under one (seed, call).
// The handle, the setter's declaration and the Philox rounds are plain C++ as well: csrc/rr_frames.hpp's host emulation includes this.
#pragma once
#include <stdint.h>
#include <stddef.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RR_DQN_HD __host__ __device__ __forceinline__
#else
#define RR_DQN_HD inline
#endif

struct rr_dqn {
    int device, nwg;
    float *partials, *m1, *m2;
    long long step;
    uint32_t *chunk_off; // rr_dqn_store's per-chunk offsets (grown on demand; a call with a larger batch than any before allocates)
    size_t chunk_cap;
    uint16_t *cnn_weights; // rr_cnn_act's bf16 copy of the weights, rewritten by every call (allocated by the first)
    float *sac_partials;   // rr_sac_grads' per-(net, chunk) partial gradients (allocated by the first call, grown by a call that needs more slots)
    size_t sac_cap;        // ... its size in slots
};

// sets the string rr_dqn_last_error returns (thread-local, rr_dqn.hip) and hands `code` back
__attribute__((visibility("hidden"))) int rr_dqn_fail(int code, const char *msg);

RR_DQN_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
#if defined(__HIPCC__)
// the action of row `row` in call `call`: the greedy one, or (np.random.random() <= epsilon: explore) a uniform one
__device__ __forceinline__ int epsilon_greedy(int best, int row, uint32_t call, uint64_t seed, float epsilon) {
    if (epsilon > 0.0f) {
        uint32_t r[4] = { (uint32_t)row, call, 0x0AC7u, 0u };
        philox4x32_10(r, (uint32_t)seed, (uint32_t)(seed >> 32));
        if ((float)r[0] * 2.3283064365386963e-10f <= epsilon) best = (int)(r[1] & 7u);
    }
    return best;
}
#endif
