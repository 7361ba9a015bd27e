// rr_frames_emu.cpp -- host emulation of the frame-sharing replay's two kernels: compiles roborugby_amd/csrc/rr_frames.hpp with g++ and
// walks k_frames_push's and k_frames_sample's grids (workgroups x 256 threads) on the host; the workgroup's decision -- 16 lanes and a
// ballot on the device -- is the loop over the same attempts, lowest first.  TEST HARNESS ONLY: the CPU suite compares the kernels' own
// arithmetic and guards with tests/frames_ref.py without a GPU.  The product library never links or loads this.  With
// -DRR_FRAMES_EMU_MAIN it is a stand-alone program (for a sanitizer build: every ring and output is a heap block of exactly its size).
#include "../../roborugby_amd/csrc/rr_frames.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace rr;

extern "C" {
int frames_push_emu(const uint8_t *src, int64_t src_row_stride, const uint8_t *first, const int32_t *action, const float *reward,
                    const uint8_t *done, const uint8_t *valid, int32_t rows, int64_t frame_bytes, int64_t slots, int64_t head, uint8_t *frames,
                    uint8_t *age, int32_t *action_ring, float *reward_ring, uint8_t *flags) {
    const FramesPush P = { src, src_row_stride, first, action, reward, done, valid, rows, frame_bytes, slots, head, frames, age, action_ring, reward_ring, flags };
    if (frames_push_refusal(P)) return -1;
    const int64_t blocks = (int64_t)rows * frames_chunks(frame_bytes);
    for (int64_t bx = 0; bx < blocks; bx++)
        for (int t = 0; t < FRAMES_THREADS; t++) frames_push_thread(P, bx, t);
    return 0;
}

int frames_sample_emu(const uint8_t *frames, const uint8_t *age, const int32_t *action_ring, const float *reward_ring, const uint8_t *flags,
                      int32_t rows, int64_t frame_bytes, int64_t slots, int64_t head, int32_t stack, int32_t batch, const int64_t *index,
                      uint64_t seed, uint32_t call, uint8_t *state, uint8_t *next_state, int32_t *action, float *reward, uint8_t *terminal,
                      uint8_t *ok, int64_t *picked) {
    const FramesSample S = { frames, age, action_ring, reward_ring, flags, rows, frame_bytes, slots, head, stack, batch, index, seed, call,
                             state, next_state, action, reward, terminal, ok, picked };
    if (frames_sample_refusal(S)) return -1;
    const int chunks = (int)frames_chunks(frame_bytes);
    for (int64_t bx = 0; bx < (int64_t)batch * chunks; bx++) {
        const int b = (int)(bx / chunks), chunk = (int)(bx % chunks);
        FramesPick decided, mine;
        memset(&decided, 0xFF, sizeof decided); // (LDS starts out undefined)
        bool any = false;
        for (int t = 0; t < 64 && !any; t++) { // the first wavefront; the ballot's lowest set lane
            bool accepted = false;
            if (index) {
                if (t == 0) accepted = frames_explicit(S, b, mine);
            } else if (t < FRAMES_ATTEMPTS) {
                accepted = frames_attempt(S, b, t, mine);
            }
            if (accepted) {
                frames_reach(S, mine);
                decided = mine;
                any = true;
            }
        }
        if (!any) frames_no_pick(decided);
        for (int t = 0; t < FRAMES_THREADS; t++) {
            if (chunk == 0 && t == 0) frames_sample_meta(S, b, decided);
            frames_sample_piece(S, b, (int64_t)chunk * FRAMES_THREADS + t, decided);
        }
    }
    return 0;
}
}

#ifdef RR_FRAMES_EMU_MAIN
// Rings of several shapes, pushed past three wraps from a strided source with random first / valid / done, then sampled with every explicit
// index around the window and in draw mode.  Every block is malloc'ed at exactly its size: a byte outside it is a heap overflow.
static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

template <class T> static T *block(size_t n, int fill) {
    T *p = (T *)malloc(n * sizeof(T) ? n * sizeof(T) : 1);
    memset(p, fill, n * sizeof(T));
    return p;
}

int main() {
    const int64_t fbs[3] = { 16, 48, 4112 };
    const int stacks[3] = { 1, 2, 4 }, rowss[2] = { 1, 5 }, extras[2] = { 1, 3 };
    unsigned long sum = 0;
    int runs = 0;
    uint32_t seed = 12345u;
    for (int64_t fb : fbs) for (int stack : stacks) for (int extra : extras) for (int rows : rowss) {
        const int64_t slots = stack + extra, cells = slots * rows, stride = fb * stack;
        uint8_t *frames = block<uint8_t>((size_t)(cells * fb), 0xAB), *age = block<uint8_t>((size_t)cells, 0xAB), *flags = block<uint8_t>((size_t)cells, 0xAB);
        int32_t *act = block<int32_t>((size_t)cells, 0xAB);
        float *rew = block<float>((size_t)cells, 0xAB);
        for (int64_t head = 0; head < 3 * slots + 1; head++) {
            // the source: a stacked observation of exactly rows * stride bytes, its newest frame last
            uint8_t *obs = block<uint8_t>((size_t)(rows * stride), 0), *first = block<uint8_t>((size_t)rows, 0), *done = block<uint8_t>((size_t)rows, 0), *valid = block<uint8_t>((size_t)rows, 0);
            int32_t *a = block<int32_t>((size_t)rows, 0);
            float *r = block<float>((size_t)rows, 0);
            for (int64_t i = 0; i < rows * stride; i++) obs[i] = (uint8_t)lcg(seed);
            for (int i = 0; i < rows; i++) { first[i] = lcg(seed) % 10 < 3; done[i] = lcg(seed) % 5 == 0; valid[i] = lcg(seed) % 10 < 7; a[i] = (int32_t)(lcg(seed) % 8); r[i] = (float)(lcg(seed) % 100) * 0.25f; }
            const bool bare = head % 7 == 3; // a push that only records frames
            if (frames_push_emu(obs + stride - fb, stride, head % 5 == 4 ? nullptr : first, bare ? nullptr : a, bare ? nullptr : r, bare ? nullptr : done,
                                bare ? nullptr : valid, rows, fb, slots, head, frames, age, act, rew, flags))
                return 1;
            free(obs); free(first); free(done); free(valid); free(a); free(r);
            const int64_t now = head + 1;
            // explicit: every (k, row) around the window
            const int batch = (int)((now + 2) * (rows + 2));
            int64_t *index = block<int64_t>((size_t)batch * 2, 0), *picked = block<int64_t>((size_t)batch * 2, 0xAB);
            int q = 0;
            for (int64_t k = -1; k <= now; k++) for (int64_t i = -1; i <= rows; i++) { index[2 * q] = k; index[2 * q + 1] = i; q++; }
            for (int mode = 0; mode < 2; mode++) {
                if (mode == 1 && now - frames_window_lo(now, slots, stack) < 1) continue;
                uint8_t *st = block<uint8_t>((size_t)(batch * stack * fb), 0xAB), *nx = block<uint8_t>((size_t)(batch * stack * fb), 0xAB);
                uint8_t *term = block<uint8_t>((size_t)batch, 0xAB), *ok = block<uint8_t>((size_t)batch, 0xAB);
                int32_t *ao = block<int32_t>((size_t)batch, 0xAB);
                float *ro = block<float>((size_t)batch, 0xAB);
                if (frames_sample_emu(frames, age, act, rew, flags, rows, fb, slots, now, stack, batch, mode ? nullptr : index, 99u + (uint64_t)head, 7u, st, nx,
                                      ao, ro, term, ok, mode ? nullptr : picked))
                    return 1;
                for (int b = 0; b < batch; b++) {
                    if (ok[b] > 1 || term[b] > 1) { printf("ok / terminal is not 0 or 1\n"); return 1; }
                    if (!mode && ok[b] && (picked[2 * b] != index[2 * b] || picked[2 * b + 1] != index[2 * b + 1])) { printf("picked differs from the index\n"); return 1; }
                    if (!ok[b]) for (int64_t z = 0; z < stack * fb; z++) if (st[b * stack * fb + z] || nx[b * stack * fb + z]) { printf("a refused sample is not zero\n"); return 1; }
                    // the newest frame of the next state is the one push k stored
                    if (!mode && ok[b] && memcmp(nx + (b * stack + stack - 1) * fb, frames + ((picked[2 * b] % slots) * rows + picked[2 * b + 1]) * fb, (size_t)fb)) {
                        printf("the next state's newest frame is not push k's\n");
                        return 1;
                    }
                    sum += ok[b];
                }
                for (int64_t z = 0; z < batch * stack * fb; z++) sum += st[z] + nx[z];
                free(st); free(nx); free(term); free(ok); free(ao); free(ro);
                runs++;
            }
            free(index); free(picked);
        }
        free(frames); free(age); free(flags); free(act); free(rew);
    }
    // the guards refuse before anything is touched
    uint8_t byte[32] = { 0 };
    int32_t word[2] = { 0 };
    float real[2] = { 0 };
    if (frames_push_emu(nullptr, 16, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 16, 2, 0, byte, byte, word, real, byte) != -1) return 1;
    if (frames_sample_emu(byte, byte, word, real, byte, 1, 16, 2, 2, 2, 1, nullptr, 0, 0, byte, byte, word, real, byte, byte, nullptr) != -1) return 1;
    printf("rr_frames_emu: %d sampled rings done, checksum %lu\n", runs, sum);
    return 0;
}
#endif
