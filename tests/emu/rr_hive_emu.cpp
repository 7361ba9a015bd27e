// rr_hive_emu.cpp -- host-emulated wave of the hive-mind player's kernel: compiles roborugby_amd/csrc/rr_hive.hpp (and rr_sim.hpp /
// rr_extras.hpp under it) with g++, every lane-parallel phase a loop over the virtual wave's lanes.  TEST HARNESS ONLY: the CPU
// suite checks the assignment's lane -> pair map, the masked arg-min rounds and the per-robot observation against vectors recorded
// from the reference without a GPU.  The product library never links or loads this.
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

// n states in canonical layout (include/roborugby_amd.h: robots [n,NR,10], balls [n,NB,8]) -> assign [n,NR], obs [n,NR,11]
template <class C> static void run(double W, double H, int n, const double *robots, const double *balls, uint32_t mask, int kind,
                                   int32_t *assign, double *obs) {
    using R = typename C::Real;
    static Arena<C> A; // (scratch leftovers of the previous state stay, as in an LDS slice)
    SimParams<R> sp;
    fill_params(sp, W, H);
    for (int a = 0; a < n; a++) {
        for (int r = 0; r < C::NR; r++) {
            const double *q = robots + ((size_t)a * C::NR + r) * 10;
            A.p.rcx[r] = (R)q[0]; A.p.rcy[r] = (R)q[1]; A.p.rl[r] = (R)q[2]; A.p.rrt[r] = (R)q[3]; A.p.rt[r] = (R)q[4];
            A.p.rb[r] = (R)q[5]; A.p.rrot[r] = (R)q[6]; A.p.px[r] = (R)q[7]; A.p.py[r] = (R)q[8]; A.p.prot[r] = (R)q[9];
        }
        for (int b = 0; b < C::NB; b++) {
            const double *q = balls + ((size_t)a * C::NB + b) * 8;
            A.p.bcx[b] = (R)q[0]; A.p.bcy[b] = (R)q[1]; A.p.bl[b] = (R)q[2]; A.p.brt[b] = (R)q[3]; A.p.bt[b] = (R)q[4];
            A.p.bb[b] = (R)q[5]; A.p.bvx[b] = (R)q[6]; A.p.bvy[b] = (R)q[7];
        }
        derive(A, sp);
        Rec<C> q = { reinterpret_cast<const R *>(&A.p) };
        if (kind == OBS_V2) hive_observe<C, double, OBS_V2>(A, q, sp, mask, assign + (size_t)a * C::NR, obs + (size_t)a * C::NR * 11);
        else hive_observe<C, double, OBS_V1>(A, q, sp, mask, assign + (size_t)a * C::NR, obs + (size_t)a * C::NR * 11);
    }
}

extern "C" {
// preset 0 T, 1 G, 2 D, 3 X (2 + 1 robots, 2 + 3 balls); vw: lanes per arena; f32: arithmetic in fp32 (G only).  -1: not built.
int hive_emu(int preset, int vw, int f32, double W, double H, int n, const double *robots, const double *balls, uint32_t mask,
             int kind, int32_t *assign, double *obs) {
#define CASE(p_, a, b, c, d, R_, f_, v_) \
    if (preset == p_ && vw == v_ && f32 == f_) { run<Cfg<a, b, c, d, R_, v_>>(W, H, n, robots, balls, mask, kind, assign, obs); return 0; }
    CASE(0, 1, 0, 1, 0, double, 0, 2) CASE(0, 1, 0, 1, 0, double, 0, 4) CASE(0, 1, 0, 1, 0, double, 0, 64)
    CASE(1, 2, 2, 4, 4, double, 0, 8) CASE(1, 2, 2, 4, 4, double, 0, 16) CASE(1, 2, 2, 4, 4, double, 0, 32) CASE(1, 2, 2, 4, 4, double, 0, 64)
    CASE(1, 2, 2, 4, 4, float, 1, 8) CASE(1, 2, 2, 4, 4, float, 1, 64)
    CASE(2, 1, 1, 1, 1, double, 0, 4) CASE(2, 1, 1, 1, 1, double, 0, 64)
    CASE(3, 2, 1, 2, 3, double, 0, 8) CASE(3, 2, 1, 2, 3, double, 0, 64)
#undef CASE
    return -1;
}
}
