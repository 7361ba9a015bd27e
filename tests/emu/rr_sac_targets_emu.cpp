// rr_sac_targets_emu.cpp -- host emulation of rr_sac_targets' per-row arithmetic: compiles roborugby_amd/csrc/rr_sac.hpp with g++ and runs
// the gather's bounds rule, the draw on the targets' stream word and the two closing formulas row by row, as the kernel's one-lane-per-row
// epilogues do.  TEST HARNESS ONLY: the CPU suite compares the kernel's own per-row functions with tests/sac_targets_ref.py without a GPU.
// The product library never links or loads this.  With -DRR_SAC_TARGETS_EMU_MAIN it is a stand-alone program (for a sanitizer build: every
// input and output is a heap block of exactly its size).
#include "../../roborugby_amd/csrc/rr_sac.hpp"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace rr;

extern "C" {
uint32_t sac_targets_stream_emu(void) { return SAC_TARGETS_STREAM; }
// u [n, 2, 2]: (pair, (u1, u2)) of batch rows 0 .. n-1 on the targets' stream word
void sac_targets_uniforms_emu(uint64_t seed, uint32_t call, int32_t n, float *u) {
    for (int32_t row = 0; row < n; row++) {
        uint32_t w[4] = { (uint32_t)row, call, SAC_TARGETS_STREAM, 0u };
        philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
        sac_uniforms(w[0], w[1], u[4 * row + 0], u[4 * row + 1]);
        sac_uniforms(w[2], w[3], u[4 * row + 2], u[4 * row + 3]);
    }
}
// z [n, 4]: sac_draw with the stream argument; stream_default != 0: without it (rr_sac_act's word)
void sac_targets_draw_emu(uint64_t seed, uint32_t call, int32_t n, int32_t stream_default, float *z) {
    for (int32_t row = 0; row < n; row++) {
        if (stream_default) sac_draw((uint32_t)row, call, seed, z + 4 * row);
        else sac_draw((uint32_t)row, call, seed, z + 4 * row, SAC_TARGETS_STREAM);
    }
}
// ok [n] = the bounds rule of index [n] against mem_rows
void sac_ring_row_ok_emu(const int64_t *index, int32_t n, int64_t mem_rows, uint8_t *ok) {
    for (int32_t b = 0; b < n; b++) ok[b] = sac_ring_row_ok(index[b], mem_rows) ? 1 : 0;
}
// the gather and the closing formulas of a batch: batch row b takes ring row index[b] of reward [mem_rows] / terminal [mem_rows]; a row
// outside the rings is never read and gives NaN.  q1, q2, log_prob, v_next: [n] -> value_target, q_hat [n]
int sac_targets_close_emu(const int64_t *index, int32_t n, int64_t mem_rows, const float *reward, const uint8_t *terminal, const float *q1,
                          const float *q2, const float *log_prob, const float *v_next, float reward_scale, float gamma, float *value_target,
                          float *q_hat) {
    if (!index || !reward || !terminal || !q1 || !q2 || !log_prob || !v_next || !value_target || !q_hat || n <= 0 || mem_rows < 1) return -1;
    for (int32_t b = 0; b < n; b++) {
        const int64_t i = index[b];
        if (!sac_ring_row_ok(i, mem_rows)) { value_target[b] = q_hat[b] = NAN; continue; }
        value_target[b] = sac_value_target(q1[b], q2[b], log_prob[b]);
        q_hat[b] = sac_q_hat(reward_scale, reward[i], gamma, terminal[i] != 0, v_next[b]);
    }
    return 0;
}
}

#ifdef RR_SAC_TARGETS_EMU_MAIN
// Batches of several sizes over rings of several sizes, with indices at and beyond both ends of the rings.  Every block is malloc'ed at
// exactly its size: a word outside it is a heap overflow.
template <class T> static T *block(size_t n) {
    const size_t bytes = n * sizeof(T);
    T *p = (T *)malloc(bytes > 0 ? bytes : 1);
    memset(p, 0xAB, bytes);
    return p;
}

int main() {
    const uint64_t seeds[3] = { 0u, 2u, 0x1234ABCD00000002ull };
    const uint32_t calls[3] = { 1u, 7u, 0xFFFFFFFFu };
    const int32_t ns[3] = { 1, 64, 4097 };
    const int64_t rings[3] = { 1, 300, 5000 };
    double sum = 0.0;
    int runs = 0;
    for (int s = 0; s < 3; s++) for (int32_t n : ns) for (int64_t m : rings) {
        float *u = block<float>((size_t)n * 4), *z = block<float>((size_t)n * 4), *z0 = block<float>((size_t)n * 4);
        sac_targets_uniforms_emu(seeds[s], calls[s], n, u);
        sac_targets_draw_emu(seeds[s], calls[s], n, 0, z);
        sac_targets_draw_emu(seeds[s], calls[s], n, 1, z0);
        int same = 0;
        for (int32_t i = 0; i < 4 * n; i++) {
            if (!std::isfinite(z[i]) || !std::isfinite(z0[i])) { printf("a draw is not finite\n"); return 1; }
            same += z[i] == z0[i];
        }
        if (same == 4 * n) { printf("the two stream words give the same draws\n"); return 1; }
        int64_t *index = block<int64_t>((size_t)n);
        uint8_t *ok = block<uint8_t>((size_t)n), *terminal = block<uint8_t>((size_t)m);
        float *reward = block<float>((size_t)m), *q1 = block<float>((size_t)n), *q2 = block<float>((size_t)n), *lp = block<float>((size_t)n),
              *v = block<float>((size_t)n), *vt = block<float>((size_t)n), *qh = block<float>((size_t)n);
        for (int64_t i = 0; i < m; i++) { reward[i] = 0.25f * (float)(i % 17) - 2.0f; terminal[i] = i % 5 == 0; }
        for (int32_t b = 0; b < n; b++) {
            // -1 and m (outside), 0 and m - 1 (the ends), then rows inside
            index[b] = b % 7 == 3 ? -1 : b % 7 == 5 ? m : b % 7 == 0 ? 0 : b % 7 == 1 ? m - 1 : (int64_t)(u[4 * b + 1] * (float)m) % m;
            q1[b] = z[4 * b]; q2[b] = z[4 * b + 1]; lp[b] = z[4 * b + 2]; v[b] = z[4 * b + 3];
        }
        sac_ring_row_ok_emu(index, n, m, ok);
        if (sac_targets_close_emu(index, n, m, reward, terminal, q1, q2, lp, v, 2.0f, 0.99f, vt, qh)) return 1;
        for (int32_t b = 0; b < n; b++) {
            const bool in = index[b] >= 0 && index[b] < m;
            if ((ok[b] != 0) != in) { printf("bounds rule\n"); return 1; }
            if (in != std::isfinite(vt[b]) || in != std::isfinite(qh[b])) { printf("a row outside the rings is not NaN, or one inside is\n"); return 1; }
            if (in && terminal[index[b]] && qh[b] != 2.0f * reward[index[b]]) { printf("terminal row\n"); return 1; }
            if (in) sum += vt[b] + qh[b];
        }
        free(u); free(z); free(z0); free(index); free(ok); free(terminal); free(reward); free(q1); free(q2); free(lp); free(v); free(vt); free(qh);
        runs++;
    }
    float one[1] = { 0 };
    int64_t i0[1] = { 0 };
    uint8_t t0[1] = { 0 };
    if (sac_targets_close_emu(i0, 1, 0, one, t0, one, one, one, one, 2.0f, 0.99f, one, one) != -1) return 1;
    if (sac_targets_close_emu(nullptr, 1, 1, one, t0, one, one, one, one, 2.0f, 0.99f, one, one) != -1) return 1;
    printf("rr_sac_targets_emu: %d batches done, checksum %.6f\n", runs, sum);
    return 0;
}
#endif
