// rr_sac_emu.cpp -- host emulation of rr_sac_act's epilogue: compiles roborugby_amd/csrc/rr_sac.hpp with g++ and runs its draw and squash
// row by row, as the kernel's one-lane-per-row epilogue does.  TEST HARNESS ONLY: the CPU suite compares the kernel's own per-row
// functions with tests/sac_ref.py without a GPU.  The product library never links or loads this.  With -DRR_SAC_EMU_MAIN it is a
// stand-alone program (for a sanitizer build: every input and output is a heap block of exactly its size).
#include "../../roborugby_amd/csrc/rr_sac.hpp"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace rr;

extern "C" {
// u [n, 2, 2]: (pair, (u1, u2)) of rows 0 .. n-1
void sac_uniforms_emu(uint64_t seed, uint32_t call, int32_t n, float *u) {
    for (int32_t row = 0; row < n; row++) {
        uint32_t w[4] = { (uint32_t)row, call, SAC_STREAM, 0u };
        philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
        sac_uniforms(w[0], w[1], u[4 * row + 0], u[4 * row + 1]);
        sac_uniforms(w[2], w[3], u[4 * row + 2], u[4 * row + 3]);
    }
}
// z [n, 4]
void sac_draw_emu(uint64_t seed, uint32_t call, int32_t n, float *z) {
    for (int32_t row = 0; row < n; row++) sac_draw((uint32_t)row, call, seed, z + 4 * row);
}
// the epilogue's loop over a row's components: head [n, 2A] (mu, raw sigma), z [n, A] -> actions [n, A], log_prob [n]
int sac_squash_emu(const float *head, const float *z, int32_t n, int32_t A, float max_action, float *actions, float *log_prob) {
    if (!head || !z || !actions || !log_prob || n <= 0 || (A != 2 && A != 4)) return -1;
    for (int32_t row = 0; row < n; row++) {
        float lp = 0.0f;
        for (int k = 0; k < A; k++) {
            const float mu = head[(size_t)row * 2 * A + k], sigma = sac_sigma(head[(size_t)row * 2 * A + A + k]);
            const float a = sac_action(mu, sigma, z[(size_t)row * A + k], max_action);
            lp += sac_log_prob_term(sigma, z[(size_t)row * A + k], a);
            actions[(size_t)row * A + k] = a;
        }
        log_prob[row] = lp;
    }
    return 0;
}
}

#ifdef RR_SAC_EMU_MAIN
// Draws for several (seed, call) and row counts, squashed at A = 2 and 4 with heads that take both arms of the clamp.  Every block is
// malloc'ed at exactly its size: a word outside it is a heap overflow.
template <class T> static T *block(size_t n) {
    T *p = (T *)malloc(n * sizeof(T) ? n * sizeof(T) : 1);
    memset(p, 0xAB, n * sizeof(T));
    return p;
}

int main() {
    const uint64_t seeds[3] = { 0u, 2u, 0x1234ABCD00000002ull };
    const uint32_t calls[3] = { 1u, 7u, 0xFFFFFFFFu };
    const int32_t ns[3] = { 1, 64, 4097 };
    double sum = 0.0;
    int runs = 0;
    for (int s = 0; s < 3; s++) for (int32_t n : ns) {
        float *u = block<float>((size_t)n * 4), *z = block<float>((size_t)n * 4);
        sac_uniforms_emu(seeds[s], calls[s], n, u);
        sac_draw_emu(seeds[s], calls[s], n, z);
        for (int32_t i = 0; i < n; i++) {
            if (!(u[4 * i] > 0.0f && u[4 * i] <= 1.0f && u[4 * i + 2] > 0.0f && u[4 * i + 2] <= 1.0f)) { printf("u1 outside (0, 1]\n"); return 1; }
            if (!(u[4 * i + 1] >= 0.0f && u[4 * i + 1] < 1.0f && u[4 * i + 3] >= 0.0f && u[4 * i + 3] < 1.0f)) { printf("u2 outside [0, 1)\n"); return 1; }
            for (int k = 0; k < 4; k++) if (!std::isfinite(z[4 * i + k])) { printf("a draw is not finite\n"); return 1; }
        }
        for (int32_t A = 2; A <= 4; A += 2) {
            float *head = block<float>((size_t)n * 2 * A), *zz = block<float>((size_t)n * A), *act = block<float>((size_t)n * A), *lp = block<float>((size_t)n);
            for (int32_t i = 0; i < n; i++) for (int k = 0; k < A; k++) {
                head[(size_t)i * 2 * A + k] = 0.5f * z[4 * i + (k + 1) % 4];           // mu
                head[(size_t)i * 2 * A + A + k] = 2.0f * u[4 * i + k] - 0.5f;          // raw sigma in (-0.5, 1.5]: both arms
                zz[(size_t)i * A + k] = z[4 * i + k];
            }
            if (sac_squash_emu(head, zz, n, A, 1.0f, act, lp)) return 1;
            for (int32_t i = 0; i < n; i++) {
                if (!std::isfinite(lp[i])) { printf("a log-probability is not finite\n"); return 1; }
                for (int k = 0; k < A; k++) if (!(std::fabs(act[(size_t)i * A + k]) <= 1.0f)) { printf("an action outside [-1, 1]\n"); return 1; }
                sum += lp[i];
            }
            free(head); free(zz); free(act); free(lp);
            runs++;
        }
        free(u); free(z);
    }
    float one[8] = { 0 };
    if (sac_squash_emu(one, one, 1, 3, 1.0f, one, one) != -1 || sac_squash_emu(nullptr, one, 1, 2, 1.0f, one, one) != -1) return 1;
    printf("rr_sac_emu: %d squashed batches done, checksum %.6f\n", runs, sum);
    return 0;
}
#endif
