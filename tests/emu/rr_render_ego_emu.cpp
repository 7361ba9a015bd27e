// rr_render_ego_emu.cpp -- host emulation of the egocentric frame kernel: compiles roborugby_amd/csrc/rr_render.hpp with g++ and walks
// k_render_ego's grid (frames x blocks x 256 threads: draw list, camera, then the quads) on the host.  TEST HARNESS ONLY: the CPU suite
// compares the kernel's own builder, camera, shading core and byte packing with tests/render_ego_ref.py without a GPU.  The product library
// never links or loads this.  With -DRR_RENDER_EGO_EMU_MAIN it is a stand-alone program over crafted arenas (for a sanitizer build: every
// frame buffer is a heap block of exactly the frames' size).
#include "../../roborugby_amd/csrc/rr_render.hpp"
#define EMU_COMMON_RENDER // the records, the layout and the crafted arenas both render emulations use
#include "emu_common.hpp"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace rr;

// k_render_ego, block by block.  recs: n records in the canonical field order (robots [10][nr], balls [8][nb]) as floats or doubles.
static void render_ego_grid(const RenderLayout &L, const EgoView &V, const void *recs, int n, const int32_t *arenas, const int32_t *robots, int m,
                            uint8_t *rgb) {
    const size_t quads = (size_t)V.width * (size_t)V.height / RENDER_QUAD;
    const size_t blocks = (quads + RENDER_THREADS - 1) / RENDER_THREADS;
    for (size_t frame = 0; frame < (size_t)m; frame++) {
        for (size_t bx = 0; bx < blocks; bx++) {
            DrawList dl;
            memset(&dl, 0xFF, sizeof dl); // (LDS starts out undefined: NaN floats here)
            size_t arena;
            int viewer;
            bool valid = render_arena_of(arenas, frame, n, arena);
            valid = render_viewer_of(robots, frame, L.nr, viewer) && valid;
            const bool swap = render_ego_swap(L, V.flags, viewer);
            if (valid) for (int t = 0; t < RENDER_THREADS; t++) render_build_ego(L, render_record(L, recs, arena), t, swap, dl);
            EgoCamera cam = {};
            if (valid) valid = render_camera(dl, viewer, swap, cam);
            for (int t = 0; t < RENDER_THREADS; t++) {
                const size_t q = bx * RENDER_THREADS + (size_t)t;
                if (q >= quads) continue;
                uint32_t w[3];
                size_t o[3];
                render_quad_ego(dl, L.nr, L.nb, V, cam, valid, q, w[0], w[1], w[2]);
                render_quad_ego_at(V.flags, quads, q, o[0], o[1], o[2]);
                for (int k = 0; k < 3; k++) memcpy(rgb + frame * quads * 12 + o[k] * 4, &w[k], 4); // (three dword stores on the device)
            }
        }
    }
}

extern "C" {
// robots [n,nr,10], balls [n,nb,8] (canonical layout, include/roborugby_amd.h); f32rec: the records hold floats.  arenas, viewers [m] or
// null.  rgb [m,height,width,3] or, with RR_EGO_PLANAR in flags, [m,3,height,width].  -1: arguments rr_render_ego refuses.
int render_ego_emu(int f32rec, int nr, int nrh, int nb, int nbp, double W, double H, int n, const double *robots, const double *balls,
                   const int32_t *arenas, const int32_t *viewers, int m, int width, int height, int S, float span, float ahead, int flags,
                   uint8_t *rgb) {
    if (nr < 0 || nb < 0 || nr > RENDER_MAX || nb > RENDER_MAX || n < 1 || m < 1 || width < 4 || width > 1024 || (width & 3) || height < 1 ||
        height > 1024 || (S != 1 && S != 2 && S != 4) || !(span >= 16.0f && span <= 16384.0f) || !(ahead >= -8192.0f && ahead <= 8192.0f) ||
        (flags & ~(RENDER_EGO_RELATIVE | RENDER_EGO_PLANAR)) || !rgb)
        return -1;
    const RenderLayout L = emu_render_layout(nr, nrh, nb, nbp, f32rec);
    const EgoView V = render_ego_view(W, H, width, height, S, span, ahead, flags);
    emu_render_records(f32rec, n, nr, nb, robots, balls, [&](const void *recs) { render_ego_grid(L, V, recs, n, arenas, viewers, m, rgb); });
    return 0;
}
}

#ifdef RR_RENDER_EGO_EMU_MAIN
// emu_common.hpp's crafted arenas seen by every kind of viewer in them (at each rotation, next to a wall, in a corner and in a goal, a
// ball on the viewer, a NaN viewer), and frames of arenas and robots out of range.
int main() {
    const int nr = EMU_CRAFTED_NR, nb = EMU_CRAFTED_NB, n = EMU_CRAFTED_N;
    std::vector<double> robots, balls;
    emu_crafted_arenas(robots, balls);
    const int m = 12;
    //                       zero frames: arena -1, arena 3, robot -1, robot 4, NaN x, NaN rot, INT32 min / max
    const int32_t arenas[m] = { 2, 0, 0, 1, 2, 2, -1, 3, 0, 0, 1, 1 }, viewers[m] = { 0, 3, 1, 2, 2, 1, 0, 0, -1, 4, 1, 3 };
    const int32_t wild_a[2] = { INT32_MIN, INT32_MAX }, wild_r[2] = { INT32_MAX, INT32_MIN };
    const int sizes[3][2] = { { 4, 1 }, { 64, 48 }, { 96, 96 } }, samples[2] = { 1, 4 };
    const float views[3][2] = { { 400.0f, 0.0f }, { 400.0f, 100.0f }, { 4096.0f, -60.0f } };
    unsigned long sum = 0;
    int runs = 0;
    for (int f32rec = 0; f32rec < 2; f32rec++)
        for (auto &wh : sizes)
            for (int S : samples)
                for (auto &sv : views)
                    for (int flags = 0; flags < 4; flags++) {
                        const size_t fb = (size_t)wh[0] * wh[1] * 3, bytes = m * fb;
                        uint8_t *rgb = (uint8_t *)malloc(bytes); // exactly the frames: a byte past them is a heap overflow
                        memset(rgb, 0xAB, bytes);
                        if (render_ego_emu(f32rec, nr, 2, nb, 4, 800.0, 800.0, n, robots.data(), balls.data(), arenas, viewers, m, wh[0], wh[1], S,
                                           sv[0], sv[1], flags, rgb))
                            return 1;
                        for (size_t k = 6 * fb; k < bytes; k++) if (rgb[k]) { printf("frame %zu of a bad index or viewer is not zero\n", k / fb); return 1; }
                        for (size_t f = 0; f < 6; f++) {
                            bool any = false;
                            for (size_t k = 0; k < fb; k++) any = any || rgb[f * fb + k] != 0;
                            if (!any) { printf("frame %zu is all zero\n", f); return 1; }
                        }
                        for (size_t k = 0; k < bytes; k++) sum += rgb[k];
                        free(rgb);
                        uint8_t *two = (uint8_t *)malloc(2 * fb);
                        memset(two, 0xAB, 2 * fb);
                        if (render_ego_emu(f32rec, nr, 2, nb, 4, 800.0, 800.0, n, robots.data(), balls.data(), wild_a, wild_r, 2, wh[0], wh[1], S,
                                           sv[0], sv[1], flags, two))
                            return 1;
                        for (size_t k = 0; k < 2 * fb; k++) if (two[k]) { printf("wild index: frame not zero\n"); return 1; }
                        free(two);
                        runs++;
                    }
    printf("rr_render_ego_emu: %d runs over crafted arenas done, checksum %lu\n", runs, sum);
    return 0;
}
#endif
