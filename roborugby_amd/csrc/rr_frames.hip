// rr_frames.hip -- the frame-sharing pixel replay's two launches and their C-ABI entries (include/roborugby_amd.h: rr_frames_push,
// rr_frames_sample).  What the threads do is csrc/rr_frames.hpp; here: the grids, the workgroup's decision through LDS, the guards' return.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/roborugby_amd.h"
#include "rr_frames.hpp"

namespace {

using namespace rr;

__global__ __launch_bounds__(FRAMES_THREADS) void k_frames_push(FramesPush P) { frames_push_thread(P, (int64_t)blockIdx.x, (int)threadIdx.x); }

__global__ __launch_bounds__(FRAMES_THREADS) void k_frames_sample(FramesSample S, int chunks) {
    __shared__ FramesPick decided;
    const int t = threadIdx.x, b = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    if (t < 64) { // the first wavefront decides: the attempts are independent, the lowest accepted one wins
        FramesPick mine;
        bool accepted = false;
        if (S.index) {
            if (t == 0) accepted = frames_explicit(S, b, mine);
        } else if (t < FRAMES_ATTEMPTS) {
            accepted = frames_attempt(S, b, t, mine);
        }
        const unsigned long long votes = __ballot(accepted);
        if (votes == 0ull) {
            if (t == 0) frames_no_pick(decided);
        } else if (t == __ffsll(votes) - 1) {
            frames_reach(S, mine);
            decided = mine;
        }
    }
    __syncthreads();
    const FramesPick pick = decided;
    if (chunk == 0 && t == 0) frames_sample_meta(S, b, pick);
    frames_sample_piece(S, b, (int64_t)chunk * FRAMES_THREADS + t, pick);
}

struct OnDevice { // the handle's device for the launch, the caller's afterwards
    int prev = -1;
    bool sw;
    explicit OnDevice(int device) { sw = hipGetDevice(&prev) == hipSuccess && prev != device && hipSetDevice(device) == hipSuccess; }
    ~OnDevice() { if (sw) (void)hipSetDevice(prev); }
};

int launched() {
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? rr_dqn_fail(-2, hipGetErrorString(e)) : 0;
}

int refuse(const char *entry, const char *why) { // (rr_dqn_fail copies the string)
    char msg[192];
    snprintf(msg, sizeof msg, "%s: %s", entry, why);
    return rr_dqn_fail(-1, msg);
}

} // namespace

extern "C" int rr_frames_push(rr_dqn *d, const uint8_t *src, int64_t src_row_stride, const uint8_t *first, const int32_t *action, const float *reward,
                              const uint8_t *done, const uint8_t *valid, int32_t rows, int64_t frame_bytes, int64_t slots, int64_t head,
                              uint8_t *frames, uint8_t *age, int32_t *action_ring, float *reward_ring, uint8_t *flags, void *stream) {
    if (!d) return refuse("rr_frames_push", "null handle");
    const FramesPush P = { src, src_row_stride, first, action, reward, done, valid, rows, frame_bytes, slots, head, frames, age, action_ring, reward_ring, flags };
    if (const char *why = frames_push_refusal(P)) return refuse("rr_frames_push", why);
    OnDevice on(d->device);
    const int64_t blocks = (int64_t)rows * frames_chunks(frame_bytes); // <= 2^22 * 2^8
    hipLaunchKernelGGL(k_frames_push, dim3((unsigned)blocks), dim3(FRAMES_THREADS), 0, (hipStream_t)stream, P);
    return launched();
}

extern "C" int rr_frames_sample(rr_dqn *d, const uint8_t *frames, const uint8_t *age, const int32_t *action_ring, const float *reward_ring,
                                const uint8_t *flags, int32_t rows, int64_t frame_bytes, int64_t slots, int64_t head, int32_t stack, int32_t batch,
                                const int64_t *index, uint64_t seed, uint32_t call, uint8_t *state, uint8_t *next_state, int32_t *action,
                                float *reward, uint8_t *terminal, uint8_t *ok, int64_t *picked, void *stream) {
    if (!d) return refuse("rr_frames_sample", "null handle");
    const FramesSample S = { frames, age, action_ring, reward_ring, flags, rows, frame_bytes, slots, head, stack, batch, index, seed, call,
                             state, next_state, action, reward, terminal, ok, picked };
    if (const char *why = frames_sample_refusal(S)) return refuse("rr_frames_sample", why);
    OnDevice on(d->device);
    const int chunks = (int)frames_chunks(frame_bytes);
    const int64_t blocks = (int64_t)batch * chunks; // <= 2^20 * 2^8
    hipLaunchKernelGGL(k_frames_sample, dim3((unsigned)blocks), dim3(FRAMES_THREADS), 0, (hipStream_t)stream, S, chunks);
    return launched();
}
