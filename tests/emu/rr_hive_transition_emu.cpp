// rr_hive_transition_emu.cpp -- host-emulated wave of the hive's transition kernel: compiles roborugby_amd/csrc/rr_hive.hpp
// (hive_transition, and extras_begin of rr_extras.hpp for the on_step_begin snapshot) with g++, every lane-parallel phase a loop over
// the virtual wave's lanes.  TEST HARNESS ONLY: the CPU suite holds the per-robot reward to the reference's team reward where the two
// coincide, and the validity rules, without a GPU.  The product library never links or loads this.
#include "../../roborugby_amd/csrc/rr_hive.hpp"
#include "emu_common.hpp"
#include <cmath>
#include <cstdlib>
#include <cstring>

using namespace rr;

// n transitions in canonical layout (include/roborugby_amd.h: robots [n,NR,10], balls [n,NB,8]): the state before the step (the
// snapshot is extras_begin of it, as k_extras_begin takes it) and after it (the record)
template <class C> static void run(double W, double H, int n, const double *robots0, const double *balls0, const double *robots1,
                                   const double *balls1, uint32_t mask, int kind, const int32_t *assign, const int32_t *status,
                                   const uint8_t *done, double *next_obs, double *reward, uint8_t *terminal, uint8_t *valid) {
    using R = typename C::Real;
    static Arena<C> A; // (scratch leftovers of the previous state stay, as in an LDS slice)
    SimParams<R> sp;
    emu_fill_params(sp, W, H);
    Rec<C> q = { reinterpret_cast<const R *>(&A.p) };
    R xs[xs_stride<C>()];
    for (int a = 0; a < n; a++) {
        emu_put_state(A, robots0 + (size_t)a * C::NR * 10, balls0 + (size_t)a * C::NB * 8);
        extras_begin<C>(q, xs);
        emu_put_state(A, robots1 + (size_t)a * C::NR * 10, balls1 + (size_t)a * C::NB * 8);
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
// (preset, vw, f32): a row of EMU_HIVE_TABLE.  -1: not built.
int hive_transition_emu(int preset, int vw, int f32, double W, double H, int n, const double *robots0, const double *balls0,
                        const double *robots1, const double *balls1, uint32_t mask, int kind, const int32_t *assign, const int32_t *status,
                        const uint8_t *done, double *next_obs, double *reward, uint8_t *terminal, uint8_t *valid) {
    return emu_hive_dispatch(preset, vw, f32, [&](auto c) {
        run<decltype(c)>(W, H, n, robots0, balls0, robots1, balls1, mask, kind, assign, status, done, next_obs, reward, terminal, valid);
    });
}
}
