// emu_common.hpp -- what the host emulations of tests/emu share: the copy between the canonical state layout and an arena, the hive
// emulations' parameters and table of built configurations, and (under EMU_COMMON_RENDER) the render emulations' records and crafted
// arenas.  TEST HARNESS ONLY.  rr_frames_emu.cpp needs none of it and does not include it.
#pragma once
#include "../../roborugby_amd/csrc/rr_sim.hpp"
#include <cstring>

// one state in canonical layout (include/roborugby_amd.h: robots [NR,10], balls [NB,8]; ri [NR,3] = mc / thl / thr, or null) -> the
// arena's persistent part, and back
template <class C> static inline void emu_put_state(rr::Arena<C> &A, const double *robots, const double *balls, const int32_t *ri = nullptr) {
    using R = typename C::Real;
    for (int r = 0; r < C::NR; r++) {
        const double *q = robots + 10 * r;
        A.p.rcx[r] = (R)q[0]; A.p.rcy[r] = (R)q[1]; A.p.rl[r] = (R)q[2]; A.p.rrt[r] = (R)q[3]; A.p.rt[r] = (R)q[4];
        A.p.rb[r] = (R)q[5]; A.p.rrot[r] = (R)q[6]; A.p.px[r] = (R)q[7]; A.p.py[r] = (R)q[8]; A.p.prot[r] = (R)q[9];
        if (ri) { A.i.mc[r] = ri[3 * r]; A.i.thl[r] = ri[3 * r + 1]; A.i.thr[r] = ri[3 * r + 2]; }
    }
    for (int b = 0; b < C::NB; b++) {
        const double *q = balls + 8 * b;
        A.p.bcx[b] = (R)q[0]; A.p.bcy[b] = (R)q[1]; A.p.bl[b] = (R)q[2]; A.p.brt[b] = (R)q[3]; A.p.bt[b] = (R)q[4];
        A.p.bb[b] = (R)q[5]; A.p.bvx[b] = (R)q[6]; A.p.bvy[b] = (R)q[7];
    }
}
template <class C> static inline void emu_get_state(const rr::Arena<C> &A, double *robots, double *balls, int32_t *ri = nullptr) {
    for (int r = 0; r < C::NR; r++) {
        double *q = robots + 10 * r;
        q[0] = A.p.rcx[r]; q[1] = A.p.rcy[r]; q[2] = A.p.rl[r]; q[3] = A.p.rrt[r]; q[4] = A.p.rt[r]; q[5] = A.p.rb[r];
        q[6] = A.p.rrot[r]; q[7] = A.p.px[r]; q[8] = A.p.py[r]; q[9] = A.p.prot[r];
        if (ri) { ri[3 * r] = A.i.mc[r]; ri[3 * r + 1] = A.i.thl[r]; ri[3 * r + 2] = A.i.thr[r]; }
    }
    for (int b = 0; b < C::NB; b++) {
        double *q = balls + 8 * b;
        q[0] = A.p.bcx[b]; q[1] = A.p.bcy[b]; q[2] = A.p.bl[b]; q[3] = A.p.brt[b]; q[4] = A.p.bt[b]; q[5] = A.p.bb[b];
        q[6] = A.p.bvx[b]; q[7] = A.p.bvy[b];
    }
}

// the parameters the hive emulations run under: an endless game in mode 1 (rr_emu.cpp sets the rest from its caller's)
template <typename R> static inline void emu_fill_params(rr::SimParams<R> &sp, double W, double H) {
    memset(&sp, 0, sizeof sp);
    rr::derive_constants(sp, W, H);
    sp.game_len = 1 << 30; sp.game_mode = 1; sp.memo = 1;
}

// The configurations the hive emulations are built for: X(preset, NRH, NRG, NBP, NBN, precision, f32, lanes per arena).
// preset 0 T, 1 G, 2 D, 3 X (2 + 1 robots, 2 + 3 balls), 5 W (1 + 1, 4 + 7: 11 balls at 16 lanes), 6 R (4 + 4, 2 + 2: 8 robots) -- the ids
// of tests/emu_build.py; f32: arithmetic in fp32 (G only)
#define EMU_HIVE_TABLE(X)                                                                                                             \
    X(0, 1, 0, 1, 0, double, 0, 2) X(0, 1, 0, 1, 0, double, 0, 4) X(0, 1, 0, 1, 0, double, 0, 64)                                      \
    X(1, 2, 2, 4, 4, double, 0, 8) X(1, 2, 2, 4, 4, double, 0, 16) X(1, 2, 2, 4, 4, double, 0, 32) X(1, 2, 2, 4, 4, double, 0, 64)     \
    X(1, 2, 2, 4, 4, float, 1, 8) X(1, 2, 2, 4, 4, float, 1, 64)                                                                       \
    X(2, 1, 1, 1, 1, double, 0, 4) X(2, 1, 1, 1, 1, double, 0, 64)                                                                     \
    X(3, 2, 1, 2, 3, double, 0, 8) X(3, 2, 1, 2, 3, double, 0, 64)                                                                     \
    X(5, 1, 1, 4, 7, double, 0, 16) X(5, 1, 1, 4, 7, double, 0, 64) X(6, 4, 4, 2, 2, double, 0, 8) X(6, 4, 4, 2, 2, double, 0, 64)
// f(Cfg<...>{}) of the row (preset, vw, f32), as dispatch() of rr_kernels.hip; -1: the row is not built
template <class F> static inline int emu_hive_dispatch(int preset, int vw, int f32, F &&f) {
#define X(p_, a, b, c, d, R_, f_, v_) \
    if (preset == p_ && vw == v_ && f32 == f_) { f(rr::Cfg<a, b, c, d, R_, v_>{}); return 0; }
    EMU_HIVE_TABLE(X)
#undef X
    return -1;
}

#ifdef EMU_COMMON_RENDER // the two render emulations
#include "../../roborugby_amd/csrc/rr_render.hpp"
#include <cstdlib>
#include <vector>

static inline rr::RenderLayout emu_render_layout(int nr, int nrh, int nb, int nbp, int f32rec) {
    return { 0, nr, 6 * nr, 10 * nr, 10 * nr + nb, 10 * nr + 8 * nb, nr, nrh, nb, nbp, f32rec ? 0 : 1 };
}
// robots [n,nr,10], balls [n,nb,8] (canonical layout) -> n records in the canonical field order (robots [10][nr], balls [8][nb]), as
// floats when f32rec; f(recs) runs over them
template <class F> static inline void emu_render_records(int f32rec, int n, int nr, int nb, const double *robots, const double *balls, F &&f) {
    const int stride = 10 * nr + 8 * nb;
    std::vector<double> rd((size_t)n * stride);
    for (int a = 0; a < n; a++) {
        double *rec = rd.data() + (size_t)a * stride;
        for (int r = 0; r < nr; r++) for (int k = 0; k < 10; k++) rec[k * nr + r] = robots[((size_t)a * nr + r) * 10 + k];
        for (int b = 0; b < nb; b++) for (int k = 0; k < 8; k++) rec[10 * nr + k * nb + b] = balls[((size_t)a * nb + b) * 8 + k];
    }
    if (f32rec) {
        std::vector<float> rf(rd.begin(), rd.end());
        f((const void *)rf.data());
    } else {
        f((const void *)rd.data());
    }
}
// The stand-alone programs' crafted arenas of G's shape (2 + 2 robots, 4 + 4 balls, 800 x 800): robots at rot 0, 45, 90, 200, 270 and
// 359.999 at non-integer centres, next to a wall, in a corner and across a goal edge, a ball on a robot, robot 1 over robot 0, a ball
// clipped by the frame, a consumed ball, a NaN robot.
constexpr int EMU_CRAFTED_N = 3, EMU_CRAFTED_NR = 4, EMU_CRAFTED_NB = 8;
static inline void emu_crafted_arenas(std::vector<double> &robots, std::vector<double> &balls) {
    const int nr = EMU_CRAFTED_NR, nb = EMU_CRAFTED_NB, n = EMU_CRAFTED_N;
    const double nan = strtod("nan", nullptr);
    robots.assign((size_t)n * nr * 10, 0.0);
    balls.assign((size_t)n * nb * 8, 0.0);
    const double R[n][nr][3] = { { { 300.25, 400.5, 0 }, { 310.75, 410.125, 45 }, { 500.5, 200.25, 90 }, { 120.3, 119.6, 359.999 } },
                                 { { 700.4, 690.2, 30 }, { nan, 300, 10 }, { 20.5, 780.5, 200 }, { 400, 400, nan } },
                                 { { 11.5, 21.5, 0 }, { 788.5, 778.5, 180 }, { 400.1, 21, 270 }, { 21, 400.9, 90 } } };
    const double B[n][nb][2] = { { { 300.25, 400.5 }, { 3, 300.5 }, { -1000, 50 }, { 600.5, 600.5 }, { 602.5, 603 }, { 797, 100 }, { 100, 797.5 }, { 50.5, 60.5 } },
                                 { { 700, 690 }, { nan, 5 }, { 7, 7 }, { 793, 793 }, { 400, -3 }, { 400, 803 }, { 150.2, 89.9 }, { 650, 710 } },
                                 { { 7.5, 7.5 }, { 792.5, 792.5 }, { 400, 400 }, { 401, 401 }, { 402, 402 }, { 403, 403 }, { 404, 404 }, { 405, 405 } } };
    for (int a = 0; a < n; a++) {
        for (int r = 0; r < nr; r++) { double *q = &robots[((size_t)a * nr + r) * 10]; q[0] = R[a][r][0]; q[1] = R[a][r][1]; q[6] = R[a][r][2]; }
        for (int b = 0; b < nb; b++) { double *q = &balls[((size_t)a * nb + b) * 8]; q[0] = B[a][b][0]; q[1] = B[a][b][1]; }
    }
}
#endif
