// rr_hive_emu.cpp -- host-emulated wave of the hive-mind player's kernels: compiles roborugby_amd/csrc/rr_hive.hpp (and rr_sim.hpp /
// rr_extras.hpp under it) with g++, every lane-parallel phase a loop over the virtual wave's lanes.  TEST HARNESS ONLY: the CPU
// suite checks the assignment's lane -> pair map, the masked arg-min rounds and the per-robot observation against vectors recorded
// from the reference, and which cells the held-row kernels (the hive under the budgeted step: hive_hold + hive_observe as k_hive_held
// runs them, hive_commit as k_hive_commit, hive_idle as the held transition kernel) may write, without a GPU.  The product library
// never links or loads this.
#include "../../roborugby_amd/csrc/rr_hive.hpp"
#include "emu_common.hpp"
#include <cmath>
#include <cstdlib>
#include <cstring>

using namespace rr;

// n states in canonical layout (include/roborugby_amd.h: robots [n,NR,10], balls [n,NB,8]) -> assign [n,NR], obs [n,NR,11].
// HELD (the body of k_hive_held per arena): parked [n] says whose record carries the parked mark, which is read from the record's int part
// BEFORE anything else of the record; held [n] tells which arenas' rows were left as they were.
template <class C, bool HELD> static void run(double W, double H, int n, const double *robots, const double *balls, const uint8_t *parked,
                                              uint32_t mask, int kind, int32_t *assign, double *obs, uint8_t *held) {
    using R = typename C::Real;
    static Arena<C> A; // (scratch leftovers of the previous state stay, as in an LDS slice; one arena each for the two bodies)
    SimParams<R> sp;
    emu_fill_params(sp, W, H);
    for (int a = 0; a < n; a++) {
        emu_put_state(A, robots + (size_t)a * C::NR * 10, balls + (size_t)a * C::NB * 8);
        if constexpr (HELD) {
            A.i.fzp = parked[a] ? FZP_PARKED | 5 : 5; // (the low bits are the park format's own: only bit 31 is the mark)
            if (hive_hold<C>(reinterpret_cast<const int32_t *>(&A.i), held + a)) continue;
        }
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
// (preset, vw, f32): a row of EMU_HIVE_TABLE; the held-row entries run the fp64 rows.  -1: not built.
int hive_emu(int preset, int vw, int f32, double W, double H, int n, const double *robots, const double *balls, uint32_t mask,
             int kind, int32_t *assign, double *obs) {
    return emu_hive_dispatch(preset, vw, f32, [&](auto c) { run<decltype(c), false>(W, H, n, robots, balls, nullptr, mask, kind, assign, obs, nullptr); });
}
int hive_held_emu(int preset, int vw, double W, double H, int n, const double *robots, const double *balls, const uint8_t *parked,
                  uint32_t mask, int kind, int32_t *assign, double *obs, uint8_t *held) {
    return emu_hive_dispatch(preset, vw, 0, [&](auto c) { run<decltype(c), true>(W, H, n, robots, balls, parked, mask, kind, assign, obs, held); });
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
    return emu_hive_dispatch(preset, vw, 0, [&](auto c) { idle<decltype(c)>(n, status, next_obs, reward, terminal, valid, wrote); });
}
}
