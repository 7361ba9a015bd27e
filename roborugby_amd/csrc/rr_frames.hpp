// rr_frames.hpp -- the frame-sharing pixel replay: a ring of `slots` time slots x `rows` rows that holds every frame ONCE, and the gather
// that rebuilds the two stacked observations of a transition from at most stack + 1 distinct frames.  C-ABI and the specification:
// rr_frames_push / rr_frames_sample in include/roborugby_amd.h; the __global__ wrappers and the entries: rr_frames.hip.
//
// Everything that decides anything is RR_HD here -- the slot and age arithmetic, the draw, the source-to-destination map, the guards -- so
// the same source compiles with g++ (tests/emu/rr_frames_emu.cpp walks both grids on the host).
//
//   push     grid = rows x ceil(pieces / 256) workgroups of 256 threads, a piece = 16 bytes of the row's frame: one 16-byte load and one
//            16-byte store per thread (the shape of the HBM copy probe); thread 0 of a row's first workgroup writes the row's four
//            metadata words.  Only `age` of the slot before is read from the ring.
//   sample   grid = batch x ceil(pieces / 256) workgroups of 256 threads.  Every workgroup decides its sample's (k, row, a0, a1) itself
//            (draw mode: the 16 attempts on 16 lanes and one ballot; 16 Philox calls and flag bytes are nothing next to the pixels), then
//            every thread loads its piece of the distinct source frames k - stack .. k that some destination needs -- all loads first --
//            and stores each to every slot of the two stacks that maps to it.  Uniform per workgroup, no atomics, no LDS for the pixels.
// All offsets are 64-bit: a ring is larger than 4 GiB in real use.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "rr_dqn_shared.hpp"

#ifndef RR_HD
#if defined(__HIPCC__)
#define RR_HD __host__ __device__ __forceinline__
#else
#define RR_HD inline
#endif
#endif

namespace rr {

constexpr int FRAMES_THREADS = 256, FRAMES_PIECE = 16, FRAMES_ATTEMPTS = 16, FRAMES_MAX_STACK = 8;
constexpr uint32_t FRAMES_STREAM = 0x5A3Eu; // counter word 2 of the sampler's draws
constexpr int FRAMES_VALID = 1, FRAMES_TERMINAL = 2;

#if defined(__HIPCC__)
typedef uint4 frames_piece;
#else
struct alignas(16) frames_piece { uint32_t x, y, z, w; };
#endif

struct FramesPush {
    const uint8_t *src;
    int64_t src_row_stride;
    const uint8_t *first;
    const int32_t *action;
    const float *reward;
    const uint8_t *done, *valid;
    int32_t rows;
    int64_t frame_bytes, slots, head;
    uint8_t *frames, *age;
    int32_t *action_ring;
    float *reward_ring;
    uint8_t *flags;
};

struct FramesSample {
    const uint8_t *frames, *age;
    const int32_t *action_ring;
    const float *reward_ring;
    const uint8_t *flags;
    int32_t rows;
    int64_t frame_bytes, slots, head;
    int32_t stack, batch;
    const int64_t *index;
    uint64_t seed;
    uint32_t call;
    uint8_t *state, *next_state;
    int32_t *action;
    float *reward;
    uint8_t *terminal, *ok;
    int64_t *picked;
};

// the transition a sample resolved to: push k of row `row`; m0 / m1: how many frames back the state (at k - 1) / the next state (at k)
// reach, min(stack - 1, age); sk = k % slots.  k < 0: no transition (ok = 0)
struct FramesPick {
    int64_t k, sk;
    int32_t row, m0, m1;
};

RR_HD int64_t frames_chunks(int64_t frame_bytes) { return (frame_bytes / FRAMES_PIECE + FRAMES_THREADS - 1) / FRAMES_THREADS; }
// the oldest push whose transition is still whole in the ring: the state at k - 1 reaches back to k - stack, which must not be overwritten
RR_HD int64_t frames_window_lo(int64_t head, int64_t slots, int stack) {
    const int64_t lo = head - slots + stack;
    return lo > 1 ? lo : 1;
}
RR_HD int frames_min(int a, int b) { return a < b ? a : b; }

// ---- guards: the message of the refusal, or null
inline const char *frames_ring_refusal(int32_t rows, int64_t frame_bytes, int64_t slots, int64_t head, const void *frames) {
    if (rows < 1 || rows > (1 << 22)) return "the number of rows must be in 1 .. 1<<22";
    if (frame_bytes < 16 || frame_bytes > (1 << 20) || frame_bytes % 16) return "frame_bytes must be a multiple of 16 in 16 .. 1 MiB";
    if (slots < 2 || slots > ((int64_t)1 << 31)) return "slots must be in 2 .. 1<<31";
    if (head < 0) return "head must not be negative";
    if ((uintptr_t)frames % 16) return "frames must be 16-byte aligned";
    return nullptr;
}
inline const char *frames_push_refusal(const FramesPush &P) {
    if (!P.src || !P.frames || !P.age || !P.action_ring || !P.reward_ring || !P.flags) return "null argument";
    const int given = (P.action != nullptr) + (P.reward != nullptr) + (P.done != nullptr) + (P.valid != nullptr);
    if (given != 0 && given != 4) return "action, reward, done and valid are all null or all given";
    if (const char *m = frames_ring_refusal(P.rows, P.frame_bytes, P.slots, P.head, P.frames)) return m;
    if (P.src_row_stride < P.frame_bytes || P.src_row_stride % 16 || P.src_row_stride > ((int64_t)1 << 32))
        return "src_row_stride must be a multiple of 16 in frame_bytes .. 1<<32";
    if ((uintptr_t)P.src % 16) return "src must be 16-byte aligned";
    return nullptr;
}
inline const char *frames_sample_refusal(const FramesSample &S) {
    if (!S.frames || !S.age || !S.action_ring || !S.reward_ring || !S.flags || !S.state || !S.next_state || !S.action || !S.reward || !S.terminal ||
        !S.ok)
        return "null argument";
    if (const char *m = frames_ring_refusal(S.rows, S.frame_bytes, S.slots, S.head, S.frames)) return m;
    if (S.stack < 1 || S.stack > FRAMES_MAX_STACK) return "stack must be in 1 .. 8";
    if (S.slots < S.stack + 1) return "slots must be at least stack + 1";
    if (S.batch < 1 || S.batch > (1 << 20)) return "batch must be in 1 .. 1<<20";
    if ((uintptr_t)S.state % 16 || (uintptr_t)S.next_state % 16) return "state and next_state must be 16-byte aligned";
    if (!S.index && S.head - frames_window_lo(S.head, S.slots, S.stack) < 1) return "the ring holds no transition to draw from yet";
    return nullptr;
}

// ---- push: thread t of workgroup `block`
RR_HD void frames_push_thread(const FramesPush &P, int64_t block, int t) {
    const int64_t chunks = frames_chunks(P.frame_bytes);
    const int64_t row = block / chunks, piece = (block % chunks) * FRAMES_THREADS + t;
    const int64_t slot = P.head % P.slots, cell = slot * P.rows + row;
    if (piece * FRAMES_PIECE < P.frame_bytes)
        *reinterpret_cast<frames_piece *>(P.frames + cell * P.frame_bytes + piece * FRAMES_PIECE) =
            *reinterpret_cast<const frames_piece *>(P.src + row * P.src_row_stride + piece * FRAMES_PIECE);
    if (piece == 0) {
        int a = 0;
        if (P.head > 0 && P.first && !P.first[row]) a = frames_min((int)P.age[((P.head - 1) % P.slots) * P.rows + row] + 1, 255);
        P.age[cell] = (uint8_t)a;
        P.action_ring[cell] = P.action ? P.action[row] : 0;
        P.reward_ring[cell] = P.reward ? P.reward[row] : 0.0f;
        P.flags[cell] = (uint8_t)(P.head > 0 && P.valid ? (P.valid[row] ? FRAMES_VALID : 0) | (P.done[row] ? FRAMES_TERMINAL : 0) : 0);
    }
}

// ---- sample: which transition
// (k, row) -> accepted?  Out-of-window or out-of-range values are never used as an index.
RR_HD bool frames_accept(const FramesSample &S, int64_t k, int64_t row, FramesPick &pick) {
    if (k < frames_window_lo(S.head, S.slots, S.stack) || k > S.head - 1 || row < 0 || row >= S.rows) return false;
    pick.k = k;
    pick.sk = k % S.slots;
    pick.row = (int32_t)row;
    return (S.flags[pick.sk * S.rows + row] & FRAMES_VALID) != 0;
}
// attempt a of sample b in draw mode
RR_HD bool frames_attempt(const FramesSample &S, int b, int a, FramesPick &pick) {
    uint32_t w[4] = { (uint32_t)b, S.call, FRAMES_STREAM, (uint32_t)a };
    philox4x32_10(w, (uint32_t)S.seed, (uint32_t)(S.seed >> 32));
    const int64_t lo = frames_window_lo(S.head, S.slots, S.stack);
    const int64_t k = lo + (int64_t)(((uint64_t)w[0] * (uint64_t)(S.head - lo)) >> 32);
    const int64_t row = (int64_t)(((uint64_t)w[1] * (uint64_t)S.rows) >> 32);
    return frames_accept(S, k, row, pick);
}
RR_HD bool frames_explicit(const FramesSample &S, int b, FramesPick &pick) { return frames_accept(S, S.index[2 * (int64_t)b], S.index[2 * (int64_t)b + 1], pick); }
// the reach of the two stacks of an accepted pick.  In a ring that push wrote, age[k] <= k and a frame a stack reaches is still in the ring
// (window rule); the clamp keeps any other byte pattern -- a ring that was never filled -- from becoming an index outside it.
RR_HD void frames_reach(const FramesSample &S, FramesPick &pick) {
    const int64_t oldest = S.head > S.slots ? S.head - S.slots : 0; // the oldest push the ring still holds
    const int64_t sp = pick.sk > 0 ? pick.sk - 1 : S.slots - 1;
    const int64_t r0 = pick.k - 1 - oldest, r1 = pick.k - oldest;
    int m0 = frames_min(S.stack - 1, (int)S.age[sp * S.rows + pick.row]), m1 = frames_min(S.stack - 1, (int)S.age[pick.sk * S.rows + pick.row]);
    pick.m0 = (int64_t)m0 > r0 ? (int)r0 : m0;
    pick.m1 = (int64_t)m1 > r1 ? (int)r1 : m1;
}
RR_HD void frames_no_pick(FramesPick &pick) { pick.k = -1; pick.sk = 0; pick.row = -1; pick.m0 = pick.m1 = 0; }

// the scalar outputs of sample b (one thread per sample)
RR_HD void frames_sample_meta(const FramesSample &S, int b, const FramesPick &pick) {
    const bool ok = pick.k >= 0;
    const int64_t cell = ok ? pick.sk * S.rows + pick.row : 0;
    S.action[b] = ok ? S.action_ring[cell] : 0;
    S.reward[b] = ok ? S.reward_ring[cell] : 0.0f;
    S.terminal[b] = (uint8_t)(ok && (S.flags[cell] & FRAMES_TERMINAL) ? 1 : 0);
    S.ok[b] = (uint8_t)(ok ? 1 : 0);
    if (S.picked) {
        S.picked[2 * (int64_t)b] = ok ? pick.k : -1;
        S.picked[2 * (int64_t)b + 1] = ok ? (int64_t)pick.row : -1;
    }
}

// piece `piece` (16 bytes) of both stacks of sample b.  Source d is push k - d: the next state's slot j takes d = min(stack - 1 - j, m1),
// the state's slot j takes d = 1 + min(stack - 1 - j, m0).
RR_HD void frames_sample_piece(const FramesSample &S, int b, int64_t piece, const FramesPick &pick) {
    if (piece * FRAMES_PIECE >= S.frame_bytes) return;
    const int64_t at = piece * FRAMES_PIECE, out = (int64_t)b * S.stack * S.frame_bytes + at;
    frames_piece v[FRAMES_MAX_STACK + 1];
    const frames_piece zero = { 0u, 0u, 0u, 0u };
    const bool ok = pick.k >= 0;
#pragma unroll
    for (int d = 0; d <= FRAMES_MAX_STACK; d++) {
        v[d] = zero;
        if (ok && d <= S.stack && (d <= pick.m1 || (d >= 1 && d - 1 <= pick.m0))) {
            const int64_t slot = pick.sk >= d ? pick.sk - d : pick.sk - d + S.slots;
            v[d] = *reinterpret_cast<const frames_piece *>(S.frames + (slot * S.rows + pick.row) * S.frame_bytes + at);
        }
    }
#pragma unroll
    for (int d = 0; d <= FRAMES_MAX_STACK; d++) {
#pragma unroll
        for (int j = 0; j < FRAMES_MAX_STACK; j++) {
            if (j >= S.stack) continue;
            const int dn = ok ? frames_min(S.stack - 1 - j, pick.m1) : 0, ds = ok ? 1 + frames_min(S.stack - 1 - j, pick.m0) : 0;
            if (dn == d) *reinterpret_cast<frames_piece *>(S.next_state + out + j * S.frame_bytes) = v[d];
            if (ds == d) *reinterpret_cast<frames_piece *>(S.state + out + j * S.frame_bytes) = v[d];
        }
    }
}

} // namespace rr
