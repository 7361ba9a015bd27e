// rr_hive_held_emu.cpp -- host-emulated wave of the hive's held-row kernels (the hive under the budgeted step): compiles
// roborugby_amd/csrc/rr_hive.hpp with g++ and runs hive_hold + hive_observe as k_hive_held does, hive_commit as k_hive_commit does and
// hive_idle as the held transition kernel does.  TEST HARNESS ONLY: the CPU suite checks which cells the three may write, without a
// GPU.  The product library never links or loads this.
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

// n states in canonical layout (robots [n,NR,10], balls [n,NB,8]); parked [n]: the arena's record carries the parked mark.
// The body of k_hive_held per arena: the mark is read from the record's int part BEFORE anything else of the record.
template <class C> static void run(double W, double H, int n, const double *robots, const double *balls, const uint8_t *parked, uint32_t mask,
                                   int kind, int32_t *assign, double *obs, uint8_t *held) {
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
        A.i.fzp = parked[a] ? FZP_PARKED | 5 : 5; // (the low bits are the park format's own: only bit 31 is the mark)
        if (hive_hold<C>(reinterpret_cast<const int32_t *>(&A.i), held + a)) continue;
        derive(A, sp);
        Rec<C> q = { reinterpret_cast<const R *>(&A.p) };
        if (kind == OBS_V2) hive_observe<C, double, OBS_V2>(A, q, sp, mask, assign + (size_t)a * C::NR, obs + (size_t)a * C::NR * 11);
        else hive_observe<C, double, OBS_V1>(A, q, sp, mask, assign + (size_t)a * C::NR, obs + (size_t)a * C::NR * 11);
    }
}

template <class C> static void idle(int n, const int32_t *status, double *next_obs, double *reward, uint8_t *terminal, uint8_t *valid,
                                    uint8_t *wrote) {
    for (int a = 0; a < n; a++) {
        const size_t row = (size_t)a * C::NR;
        wrote[a] = hive_idle<C, double>(status[a], next_obs + row * 11, reward + row, terminal + row, valid + row) ? 1 : 0;
    }
}

extern "C" {
// preset 0 T, 1 G; vw: lanes per arena.  -1: not built.
int hive_held_emu(int preset, int vw, double W, double H, int n, const double *robots, const double *balls, const uint8_t *parked,
                  uint32_t mask, int kind, int32_t *assign, double *obs, uint8_t *held) {
#define CASE(p_, a, b, c, d, v_) \
    if (preset == p_ && vw == v_) { run<Cfg<a, b, c, d, double, v_>>(W, H, n, robots, balls, parked, mask, kind, assign, obs, held); return 0; }
    CASE(0, 1, 0, 1, 0, 2) CASE(0, 1, 0, 1, 0, 64)
    CASE(1, 2, 2, 4, 4, 8) CASE(1, 2, 2, 4, 4, 64)
#undef CASE
    return -1;
}
// k_hive_commit's loop: one (arena, robot) cell at a time
int hive_commit_emu(int n, int nr, uint32_t mask, const int32_t *fresh, const int32_t *assign, const uint8_t *held, int32_t *accepted,
                    float *thrust) {
    for (int cell = 0; cell < n * nr; cell++) {
        const int a = cell / nr, r = cell - a * nr;
        const size_t row = (size_t)a * nr;
        hive_commit(mask, r, fresh + row, assign + row, held[a], accepted + row, thrust + 2 * row);
    }
    return 0;
}
// the early return of the held transition kernel: wrote[a] = the arena did not step and its zero rows were written
int hive_idle_emu(int preset, int vw, int n, const int32_t *status, double *next_obs, double *reward, uint8_t *terminal, uint8_t *valid,
                  uint8_t *wrote) {
    if (preset == 0 && vw == 2) { idle<Cfg<1, 0, 1, 0, double, 2>>(n, status, next_obs, reward, terminal, valid, wrote); return 0; }
    if (preset == 1 && vw == 8) { idle<Cfg<2, 2, 4, 4, double, 8>>(n, status, next_obs, reward, terminal, valid, wrote); return 0; }
    if (preset == 1 && vw == 64) { idle<Cfg<2, 2, 4, 4, double, 64>>(n, status, next_obs, reward, terminal, valid, wrote); return 0; }
    return -1;
}
}
