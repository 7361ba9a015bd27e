// rr_render_emu.cpp -- host emulation of the frame kernel: compiles roborugby_amd/csrc/rr_render.hpp with g++ and walks k_render's grid
// (frames x blocks x 256 threads: draw list, then the quads) on the host.  TEST HARNESS ONLY: the CPU suite compares the kernel's own
// draw-list builder, shading core and byte packing with tests/render_ref.py without a GPU.  The product library never links or loads this.
// With -DRR_RENDER_EMU_MAIN it is a stand-alone program over crafted arenas (for a sanitizer build: every frame buffer is a heap block
// of exactly the frames' size).
#include "../../roborugby_amd/csrc/rr_render.hpp"
#define EMU_COMMON_RENDER // the records, the layout and the crafted arenas both render emulations use
#include "emu_common.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace rr;

// k_render, block by block.  recs: n records in the canonical field order (robots [10][nr], balls [8][nb]) as floats or doubles.
static void render_grid(const RenderLayout &L, const RenderView &V, const void *recs, int n, const int32_t *arenas, int m, uint8_t *rgb) {
    const size_t quads = (size_t)V.width * (size_t)V.height / RENDER_QUAD;
    const size_t blocks = (quads + RENDER_THREADS - 1) / RENDER_THREADS;
    for (size_t frame = 0; frame < (size_t)m; frame++) {
        for (size_t bx = 0; bx < blocks; bx++) {
            DrawList dl;
            memset(&dl, 0xFF, sizeof dl); // (LDS starts out undefined: NaN floats here)
            size_t arena;
            const bool valid = render_arena_of(arenas, frame, n, arena);
            if (valid) for (int t = 0; t < RENDER_THREADS; t++) render_build(L, render_record(L, recs, arena), t, dl);
            for (int t = 0; t < RENDER_THREADS; t++) {
                const size_t q = bx * RENDER_THREADS + (size_t)t;
                if (q >= quads) continue;
                uint32_t w[3];
                render_quad(dl, L.nr, L.nb, V, valid, q, w[0], w[1], w[2]);
                memcpy(rgb + frame * quads * 12 + q * 12, w, 12); // (three dword stores on the device)
            }
        }
    }
}

extern "C" {
// robots [n,nr,10], balls [n,nb,8] (canonical layout, include/roborugby_amd.h); f32rec: the records hold floats.  arenas [m] or null.
// rgb [m,height,width,3].  -1: arguments rr_render refuses.
int render_emu(int f32rec, int nr, int nrh, int nb, int nbp, double W, double H, int n, const double *robots, const double *balls,
               const int32_t *arenas, int m, int width, int height, int S, uint8_t *rgb) {
    if (nr < 0 || nb < 0 || nr > RENDER_MAX || nb > RENDER_MAX || n < 1 || m < 1 || width < 4 || width > 4096 || (width & 3) || height < 1 ||
        height > 4096 || (S != 1 && S != 2 && S != 4) || !rgb)
        return -1;
    const RenderLayout L = emu_render_layout(nr, nrh, nb, nbp, f32rec);
    const RenderView V = { (float)W, (float)H, (float)(W / (double)(width * S)), (float)(H / (double)(height * S)), width, height, S };
    emu_render_records(f32rec, n, nr, nb, robots, balls, [&](const void *recs) { render_grid(L, V, recs, n, arenas, m, rgb); });
    return 0;
}
}

#ifdef RR_RENDER_EMU_MAIN
// emu_common.hpp's crafted arenas, framed whole at 4 x 1 and 96 x 96, S = 1 and 4, with a frame list that names arenas out of range
int main() {
    const int nr = EMU_CRAFTED_NR, nb = EMU_CRAFTED_NB, n = EMU_CRAFTED_N;
    std::vector<double> robots, balls;
    emu_crafted_arenas(robots, balls);
    const int32_t arenas[5] = { 2, 0, -1, 3, 1 };
    const int sizes[2][2] = { { 4, 1 }, { 96, 96 } }, samples[2] = { 1, 4 };
    unsigned long sum = 0;
    for (int f32rec = 0; f32rec < 2; f32rec++)
        for (auto &wh : sizes)
            for (int S : samples) {
                const size_t bytes = (size_t)5 * wh[0] * wh[1] * 3;
                uint8_t *rgb = (uint8_t *)malloc(bytes); // exactly the frames: a byte past them is a heap overflow
                memset(rgb, 0xAB, bytes);
                if (render_emu(f32rec, nr, 2, nb, 4, 800.0, 800.0, n, robots.data(), balls.data(), arenas, 5, wh[0], wh[1], S, rgb)) return 1;
                const size_t fb = bytes / 5;
                for (size_t k = 0; k < fb; k++) if (rgb[2 * fb + k] || rgb[3 * fb + k]) { printf("out-of-range frame not zero\n"); return 1; }
                for (size_t k = 0; k < bytes; k++) sum += rgb[k];
                free(rgb);
            }
    printf("rr_render_emu: 8 runs over crafted arenas done, checksum %lu\n", sum);
    return 0;
}
#endif
