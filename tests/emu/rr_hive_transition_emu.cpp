// rr_hive_transition_emu.cpp -- host-emulated wave of the hive's transition kernel: compiles roborugby_amd/csrc/rr_hive.hpp
// (hive_transition, and extras_begin of rr_extras.hpp for the on_step_begin snapshot) with g++, every lane-parallel phase a loop over
// the virtual wave's lanes.  TEST HARNESS ONLY: the CPU suite holds the per-robot reward to the reference's team reward where the two
// coincide, and the validity rules, without a GPU.  The product library never links or loads this.
#include "../../roborugby_amd/csrc/rr_hive.hpp"
#include <cmath>
#include <cstdlib>
#include <cstring>

using namespace rr;

template <typename R> static void fill_params(SimParams<R> &sp, double W, double H) {
    memset(&sp, 0, sizeof sp);
    derive_constants(sp, W, H);
    sp.game_len = 1 << 30; sp.game_mode = 1; sp.memo = 1;
}

// one state in canonical layout (include/roborugby_amd.h: robots [NR,10], balls [NB,8]) -> the arena's persistent part
template <class C> static void put(Arena<C> &A, const double *robots, const double *balls) {
    using R = typename C::Real;
    for (int r = 0; r < C::NR; r++) {
        const double *q = robots + (size_t)r * 10;
        A.p.rcx[r] = (R)q[0]; A.p.rcy[r] = (R)q[1]; A.p.rl[r] = (R)q[2]; A.p.rrt[r] = (R)q[3]; A.p.rt[r] = (R)q[4];
        A.p.rb[r] = (R)q[5]; A.p.rrot[r] = (R)q[6]; A.p.px[r] = (R)q[7]; A.p.py[r] = (R)q[8]; A.p.prot[r] = (R)q[9];
    }
    for (int b = 0; b < C::NB; b++) {
        const double *q = balls + (size_t)b * 8;
        A.p.bcx[b] = (R)q[0]; A.p.bcy[b] = (R)q[1]; A.p.bl[b] = (R)q[2]; A.p.brt[b] = (R)q[3]; A.p.bt[b] = (R)q[4];
        A.p.bb[b] = (R)q[5]; A.p.bvx[b] = (R)q[6]; A.p.bvy[b] = (R)q[7];
    }
}

// n transitions: the state before the step (the snapshot is extras_begin of it, as k_extras_begin takes it) and after it (the record)
template <class C> static void run(double W, double H, int n, const double *robots0, const double *balls0, const double *robots1,
                                   const double *balls1, uint32_t mask, int kind, const int32_t *assign, const int32_t *status,
                                   const uint8_t *done, double *next_obs, double *reward, uint8_t *terminal, uint8_t *valid) {
    using R = typename C::Real;
    static Arena<C> A; // (scratch leftovers of the previous state stay, as in an LDS slice)
    SimParams<R> sp;
    fill_params(sp, W, H);
    Rec<C> q = { reinterpret_cast<const R *>(&A.p) };
    R xs[xs_stride<C>()];
    for (int a = 0; a < n; a++) {
        put(A, robots0 + (size_t)a * C::NR * 10, balls0 + (size_t)a * C::NB * 8);
        extras_begin<C>(q, xs);
        put(A, robots1 + (size_t)a * C::NR * 10, balls1 + (size_t)a * C::NB * 8);
        derive(A, sp);
        const size_t row = (size_t)a * C::NR;
        if (kind == OBS_V2)
            hive_transition<C, double, OBS_V2>(A, q, sp, xs, mask, assign + row, status[a], done[a], next_obs + row * 11, reward + row,
                                               terminal + row, valid + row);
        else
            hive_transition<C, double, OBS_V1>(A, q, sp, xs, mask, assign + row, status[a], done[a], next_obs + row * 11, reward + row,
                                               terminal + row, valid + row);
    }
}

extern "C" {
// preset 0 T, 1 G, 2 D, 3 X (2 + 1 robots, 2 + 3 balls); vw: lanes per arena; f32: arithmetic in fp32 (G only).  -1: not built.
int hive_transition_emu(int preset, int vw, int f32, double W, double H, int n, const double *robots0, const double *balls0,
                        const double *robots1, const double *balls1, uint32_t mask, int kind, const int32_t *assign, const int32_t *status,
                        const uint8_t *done, double *next_obs, double *reward, uint8_t *terminal, uint8_t *valid) {
#define CASE(p_, a, b, c, d, R_, f_, v_)                                                                                              \
    if (preset == p_ && vw == v_ && f32 == f_) {                                                                                      \
        run<Cfg<a, b, c, d, R_, v_>>(W, H, n, robots0, balls0, robots1, balls1, mask, kind, assign, status, done, next_obs, reward,   \
                                     terminal, valid);                                                                                \
        return 0;                                                                                                                     \
    }
    CASE(0, 1, 0, 1, 0, double, 0, 2) CASE(0, 1, 0, 1, 0, double, 0, 4) CASE(0, 1, 0, 1, 0, double, 0, 64)
    CASE(1, 2, 2, 4, 4, double, 0, 8) CASE(1, 2, 2, 4, 4, double, 0, 16) CASE(1, 2, 2, 4, 4, double, 0, 32) CASE(1, 2, 2, 4, 4, double, 0, 64)
    CASE(1, 2, 2, 4, 4, float, 1, 8) CASE(1, 2, 2, 4, 4, float, 1, 64)
    CASE(2, 1, 1, 1, 1, double, 0, 4) CASE(2, 1, 1, 1, 1, double, 0, 64)
    CASE(3, 2, 1, 2, 3, double, 0, 8) CASE(3, 2, 1, 2, 3, double, 0, 64)
#undef CASE
    return -1;
}
}
