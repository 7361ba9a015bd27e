// rr_emu.cpp -- host-emulated wave: compiles roborugby_amd/csrc/rr_sim.hpp with g++ where each
// "lane-parallel" phase is a 64-iteration loop.  TEST HARNESS ONLY: it lets the CPU test-suite
// check the kernel's phase logic (lane->task maps, ballot masks, response ordering) against the
// oracle without a GPU.  The product library never links or loads this.
static int g_dbg_substeps = 12;
static int g_dbg_trace = 0;
static int g_dbg_memo = 1; // fixed-point check of the sub-step loop on/off (tests compare both)
static int g_dbg_scrub = 0; // overwrite everything but the persistent record with garbage before each step, then derive(): what a
                            // GPU launch starts from (load_record + derive into an LDS slice that holds another arena's leftovers)
#define RR_NUM_SUBSTEPS g_dbg_substeps
#define RR_EMU_TRACE g_dbg_trace
#include "../../roborugby_amd/csrc/rr_sim.hpp"
#include "../../roborugby_amd/csrc/rr_extras.hpp"
#include "emu_common.hpp"
#include <cmath>
#include <cstdlib>
#include <cstring>

using namespace rr;

template <class C> struct Emu {
    Arena<C> A;
    SimParams<typename C::Real> sp;
    Program prog;     // reward keepers in execution order (default = SimpleDuel3)
    bool custom_prog;
    uint32_t snap[Arena<C>::SNAP_WORDS];
    typename C::Real xs[xs_stride<C>()]; // on_step_begin snapshot (always taken here: AllCoords_WithPrior reads it)
    int32_t isnap[2 * C::NR];
    int goal_scoring;              // opt-in goal scoring (rr_extras.hpp: goal_step)
    int32_t gs[gs_stride<C>()];
    uint32_t park[Arena<C>::PARK_WORDS]; // budgeted step: the parked mid-step state (what the GPU keeps in its side buffer)
    uint32_t park_rng;
};

// emu_common.hpp's parameters, then what emu_create's caller chose
template <typename R> static void fill_params(SimParams<R> &sp, double W, double H, int game_len, int game_mode,
                                              int time_limit, int auto_reset, uint64_t seed) {
    emu_fill_params(sp, W, H);
    sp.game_len = game_len; sp.game_mode = game_mode; sp.time_limit = time_limit; sp.auto_reset = auto_reset & 1;
    sp.reset_on_fault = (auto_reset >> 1) & 1; // bit 1 of the flag word
    sp.seed = seed;
}

template <class C> static void set_state(Emu<C> *e, const double *robots, const int32_t *ri, const double *balls, int step) {
    Arena<C> &A = e->A;
    emu_put_state(A, robots, balls, ri);
    A.i.step = step;
    A.i.fault = 0;
    A.i.fzp = 0;
#if RR_CARRY
    A.p.ic[0] = A.p.bcx[C::NB - 1]; A.p.ic[1] = A.p.bcy[C::NB - 1]; // where a sub-step leaves the scratch rect (emu_set_scratch_rect overrides)
#endif
    derive(A, e->sp);
}

// The built kinds: X(handle kind, name, preset, mode, NRH, NRG, NBP, NBN, precision, lanes per arena).  emu_create picks the row of
// (preset, mode); every other use switches on the kind.
//   preset: the ids of tests/emu_build.py (0 T, 1 G, 2 D, 3 X, 4 Y, 5 W, 6 R, 7 Q, 8 P)
//   mode:   0 = fp64 at 64 lanes, 1 = fp32 at 64 lanes, 2 = fp64 in narrow virtual waves (names ...n): the same phases run in several
//           rounds of VW lanes (what the packed GPU builds execute)
//   D:    the duel shape (1 + 1 robots, 1 + 1 balls)
//   X:    a shape that is NOT one of the library's built ones (2 + 1 robots, 2 + 3 balls: odd counts, unequal teams): what
//         build_shape_library compiles on demand (roborugby_amd/build.py); one lane per entity needs 8 lanes
//   Y:    one that packs at FOUR lanes per arena (1 + 1 robots, 2 + 1 balls): the narrow phases' "fewer than eight lanes" variants with
//         more than one ball, a combination none of the built shapes has
//   W, R, Q, P: the shapes at the limits of rr::shape_lanes (tests/oracle_lib.py: PRESETS), each at 64 lanes and at its own width:
//         W 1 + 1 / 4 + 7 (16 lanes: 11 balls, 55 ball pairs), R 4 + 4 / 2 + 2 (8 robots, 32 ball-robot pairs), Q 2 + 2 / 3 + 3
//         (observe_both's aliasing bound at equality), P 1 + 0 / 3 + 0 (the reward scratch's bound at equality; one robot with several
//         balls, which the parity build refuses: EMU_KINDS_P is empty there)
#if RR_CARRY
#define EMU_KINDS_P(X, ...)
#else
#define EMU_KINDS_P(X, ...) X(19, CP64, 8, 0, 1, 0, 3, 0, double, 64, __VA_ARGS__) X(20, CP64n, 8, 2, 1, 0, 3, 0, double, 4, __VA_ARGS__)
#endif
#define EMU_KINDS(X, ...)                                                                                                           \
    X(0, CT64, 0, 0, 1, 0, 1, 0, double, 64, __VA_ARGS__) X(1, CG64, 1, 0, 2, 2, 4, 4, double, 64, __VA_ARGS__)                     \
    X(2, CT32, 0, 1, 1, 0, 1, 0, float, 64, __VA_ARGS__) X(3, CG32, 1, 1, 2, 2, 4, 4, float, 64, __VA_ARGS__)                       \
    X(4, CT64n, 0, 2, 1, 0, 1, 0, double, 4, __VA_ARGS__) X(5, CG64n, 1, 2, 2, 2, 4, 4, double, 16, __VA_ARGS__)                    \
    X(6, CD64, 2, 0, 1, 1, 1, 1, double, 64, __VA_ARGS__) X(7, CD32, 2, 1, 1, 1, 1, 1, float, 64, __VA_ARGS__)                      \
    X(8, CD64n, 2, 2, 1, 1, 1, 1, double, 4, __VA_ARGS__) X(9, CX64, 3, 0, 2, 1, 2, 3, double, 64, __VA_ARGS__)                     \
    X(10, CX64n, 3, 2, 2, 1, 2, 3, double, 8, __VA_ARGS__) X(11, CY64, 4, 0, 1, 1, 2, 1, double, 64, __VA_ARGS__)                   \
    X(12, CY64n, 4, 2, 1, 1, 2, 1, double, 4, __VA_ARGS__) X(13, CW64, 5, 0, 1, 1, 4, 7, double, 64, __VA_ARGS__)                   \
    X(14, CW64n, 5, 2, 1, 1, 4, 7, double, 16, __VA_ARGS__) X(15, CR64, 6, 0, 4, 4, 2, 2, double, 64, __VA_ARGS__)                  \
    X(16, CR64n, 6, 2, 4, 4, 2, 2, double, 8, __VA_ARGS__) X(17, CQ64, 7, 0, 2, 2, 3, 3, double, 64, __VA_ARGS__)                   \
    X(18, CQ64n, 7, 2, 2, 2, 3, 3, double, 8, __VA_ARGS__)                                                                          \
    EMU_KINDS_P(X, __VA_ARGS__)
#define EMU_TYPEDEF(k, name, p_, m_, a, b, c, d, R_, v_, ...) typedef Cfg<a, b, c, d, R_, v_> name;
EMU_KINDS(EMU_TYPEDEF, 0)

struct Handle { int kind; void *p; };

// runs the statements with e = the handle's Emu<CC> *
#define EMU_CASE(k, name, p_, m_, a, b, c, d, R_, v_, h, ...) case k: { auto *e = (Emu<name> *)(h)->p; typedef name CC; __VA_ARGS__; } break;
#define DISPATCH(h, ...) switch ((h)->kind) { EMU_KINDS(EMU_CASE, h, __VA_ARGS__) }

extern "C" {
void emu_debug_set_substeps(int k) { g_dbg_substeps = k; }
void emu_set_goal_scoring(Handle *h, int on) { DISPATCH(h, (e->goal_scoring = on, goal_state_clear<CC>(e->gs))); }
void emu_goal_scores(Handle *h, int32_t *s2) {
    DISPATCH(h, for (int k = 0; k < 2; k++) s2[k] = goal_score<CC>(e->gs, k));
}
void emu_debug_trace(int on) { g_dbg_trace = on; }
void emu_debug_memo(int on) { g_dbg_memo = on; }
void emu_debug_scrub(int on) { g_dbg_scrub = on; }
// primitives of the kernel source, for unit tests
double emu_py_mod360(double a) { return py_mod<double>(a, 360.0); }
void emu_sincos(double x, double *s, double *c) { m_sincos(x, *s, *c); }
// the predicate of the supported shapes as this build states it (rr_sim.hpp: shape_lanes): lanes per arena, 0 = refused
int emu_shape_lanes(int nrh, int nrg, int nbp, int nbn) { return shape_lanes(nrh, nrg, nbp, nbn, RR_CARRY != 0); }
// preset, mode: the columns of EMU_KINDS.  Null for a combination that is not built.
Handle *emu_create(int preset, int mode, double W, double H, int game_len, int game_mode, int time_limit, int auto_reset,
                   uint64_t seed) {
    int kind = -1;
#define EMU_PICK(k, name, p_, m_, ...) if (preset == p_ && mode == m_) kind = k;
    EMU_KINDS(EMU_PICK, 0)
    if (kind < 0) return nullptr;
    Handle *h = new Handle;
    h->kind = kind;
#define EMU_ALLOC(k, name, p_, m_, a, b, c, d, R_, v_, ...) case k: h->p = calloc(1, sizeof(Emu<name>)); break;
    switch (h->kind) { EMU_KINDS(EMU_ALLOC, 0) }
    DISPATCH(h, fill_params(e->sp, W, H, game_len, game_mode, time_limit, auto_reset, seed); (void)sizeof(CC);
             e->prog.n = 3; e->prog.id[0] = 1; e->prog.id[1] = 2; e->prog.id[2] = 3; e->custom_prog = false;
             for (int r = 0; r < CC::NR; r++) robot_set_clean_lane(e->A, e->sp, r, (typename CC::Real)0, (typename CC::Real)0,
                                                                   r < CC::NRH ? (typename CC::Real)90 : (typename CC::Real)-90);
             for (int b = 0; b < CC::NB; b++) ball_set_clean_lane(e->A, b, (typename CC::Real)0, (typename CC::Real)0,
                                                                  (typename CC::Real)0, (typename CC::Real)0);
             derive(e->A, e->sp));
    return h;
}
void emu_destroy(Handle *h) { free(h->p); delete h; }
void emu_set_state(Handle *h, const double *robots, const int32_t *ri, const double *balls, int step) {
    DISPATCH(h, set_state<CC>(e, robots, ri, balls, step));
}
void emu_get_state(Handle *h, double *robots, int32_t *ri, double *balls, int32_t *step) {
    DISPATCH(h, emu_get_state(e->A, robots, balls, ri); *step = e->A.i.step); // (emu_common.hpp's, on the arena)
}
// centre of the reference's scratch rect (_rectBallInner): 1 if this build carries it (the parity build), 0 otherwise
int emu_set_scratch_rect(Handle *h, const double *xy) {
#if RR_CARRY
    DISPATCH(h, e->A.p.ic[0] = (typename CC::Real)xy[0]; e->A.p.ic[1] = (typename CC::Real)xy[1]);
    return 1;
#else
    (void)h; (void)xy;
    return 0;
#endif
}
int emu_get_scratch_rect(Handle *h, double *xy) {
#if RR_CARRY
    DISPATCH(h, xy[0] = (double)e->A.p.ic[0]; xy[1] = (double)e->A.p.ic[1]);
    return 1;
#else
    (void)h; (void)xy;
    return 0;
#endif
}
void emu_set_poses(Handle *h, const double *rxyr, const double *bxyv) {
    DISPATCH(h, for (int r = 0; r < CC::NR; r++) robot_set_clean_lane(e->A, e->sp, r, (typename CC::Real)rxyr[3 * r],
                                                                   (typename CC::Real)rxyr[3 * r + 1], (typename CC::Real)rxyr[3 * r + 2]);
             for (int b = 0; b < CC::NB; b++) ball_set_clean_lane(e->A, b, (typename CC::Real)bxyv[4 * b], (typename CC::Real)bxyv[4 * b + 1],
                                                                  (typename CC::Real)bxyv[4 * b + 2], (typename CC::Real)bxyv[4 * b + 3]);
             e->A.i.step = 0; e->A.i.fzp = 0; derive(e->A, e->sp));
}
// same bracketing as rr_step: snapshot -> step kernel phases -> keeper program (only for a non-default program)
extern "C++" {
template <class CC> static void scrub_scratch(Emu<CC> *e) {
    // keep P and I (the HBM record), trash the rest of the LDS image, rebuild what the kernel derives after load_record
    typename Arena<CC>::P p = e->A.p;
    typename Arena<CC>::I i = e->A.i;
    memset(&e->A, 0xA5, sizeof(e->A));
    e->A.p = p; e->A.i = i;
    derive(e->A, e->sp);
}
// park_mod < 0: the synchronous step; >= 0: the budgeted step, parking at pseudo-random sub-step boundaries (1 in park_mod; 0 / 1: all)
template <class CC> static int emu_step_t(Emu<CC> *e, const int32_t *actions, const float *thrust, int na, double *obs,
                                          double *obs_g, double *reward, double *reward_g, uint8_t *done, int park_mod = -1) {
    using RR = typename CC::Real;
    int32_t status = 0;
    RR *xs = e->xs;
    Rec<CC> q = { reinterpret_cast<const RR *>(&e->A.p) };
    if (g_dbg_scrub) scrub_scratch(e);
    const bool was_parked = record_parked<CC>(reinterpret_cast<const int32_t *>(&e->A.i)); // (the LDS image has the record's layout: P, then I)
    if (!was_parked) extras_begin<CC>(q, xs);
    StepOut<double> o = { obs, obs_g, reward, reward_g, done, &status, g_dbg_memo ? e->snap : nullptr, e->isnap, 0, 0, 0 };
    if (park_mod >= 0) {
        ParkCtx pk;
        pk.buf = e->park; pk.host_rng = &e->park_rng; pk.host_mod = (uint32_t)park_mod;
        step_arena<CC, double, true>(e->A, e->sp, 0, actions, thrust, na, o, pk);
        if (status & ST_NOT_READY) return status;
    } else
    step_arena<CC, double>(e->A, e->sp, 0, actions, thrust, na, o);
    if (e->custom_prog && !(status & (ST_WAS_RESET | ST_STEP_AFTER_DONE))) {
        RR rh, rg;
        extras_end<CC, double>(q, e->sp, xs, e->prog, (uint32_t)status >> 16, reward, reward_g, &status, rh, rg);
    }
    if (e->goal_scoring) { // the arena's LDS image has the record's layout: P, then I
        bool bd = false;
        for (int k = 0; k < e->prog.n; k++) bd |= e->prog.id[k] == KEEPER_BASEDESTRUCTION;
        goal_step<CC, double>(reinterpret_cast<RR *>(&e->A.p), reinterpret_cast<int32_t *>(&e->A.i), e->sp, e->gs, bd, reward, reward_g, done, &status);
    }
    return status;
}
} // extern "C++"
int emu_step(Handle *h, const int32_t *actions, int na, double *obs, double *obs_g, double *reward, double *reward_g,
             uint8_t *done) {
    int32_t status = 0;
    DISPATCH(h, status = emu_step_t<CC>(e, actions, nullptr, na, obs, obs_g, reward, reward_g, done));
    return status;
}
// the budgeted step (rr_sim.hpp: ParkCtx): returns ST_NOT_READY while the step is parked; outputs are written when it completes
int emu_step_budget(Handle *h, const int32_t *actions, int na, double *obs, double *obs_g, double *reward, double *reward_g,
                    uint8_t *done, int park_mod) {
    int32_t status = 0;
    DISPATCH(h, status = emu_step_t<CC>(e, actions, nullptr, na, obs, obs_g, reward, reward_g, done, park_mod < 0 ? 0 : park_mod));
    return status;
}
void emu_park_seed(Handle *h, uint32_t seed) { DISPATCH(h, e->park_rng = seed); }
int emu_step_thrust(Handle *h, const float *thrust, int nk, double *obs, double *obs_g, double *reward, double *reward_g,
                    uint8_t *done) {
    int32_t status = 0;
    DISPATCH(h, status = emu_step_t<CC>(e, nullptr, thrust, nk, obs, obs_g, reward, reward_g, done));
    return status;
}
void emu_set_program(Handle *h, const int32_t *ids, int n) {
    DISPATCH(h, e->prog.n = n; for (int i = 0; i < n; i++) e->prog.id[i] = ids[i];
             e->custom_prog = !(n == 3 && ids[0] == 1 && ids[1] == 2 && ids[2] == 3));
}
int emu_observe_kind(Handle *h, int kind, int team, int ridx, int bidx, double *out) {
    int m = 0;
    DISPATCH(h, if (kind == 0) { int st = 0; m = observe<CC, double>(e->A, e->sp, team, ridx, bidx, out, st) ? 11 : 0; }
                else { Rec<CC> q = { reinterpret_cast<const typename CC::Real *>(&e->A.p) };
                       m = observe_kind<CC, double>(q, e->sp, kind, team, ridx, bidx, out, e->xs); });
    return m;
}
int emu_observe(Handle *h, int team, int ridx, int bidx, double *obs) {
    int st = 0, ok = 0;
    DISPATCH(h, ok = observe<CC, double>(e->A, e->sp, team, ridx, bidx, obs, st) ? 1 : 0);
    return ok;
}
int emu_reset(Handle *h, uint64_t arena, uint64_t episode) {
    int st = 0;
    DISPATCH(h, (reset_arena(e->A, e->sp, arena, episode, st), goal_state_clear<CC>(e->gs)));
    return st;
}
}
