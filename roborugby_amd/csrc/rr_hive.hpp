// rr_hive.hpp -- the reference's "hive mind" player (DQN_pytorch_player.py: Stephen.__ponder + the observation __consult asks for),
// one virtual wave per arena: which ball each hive robot goes for, and that robot's observation of that ball.
//
// __ponder (DQN_pytorch_player.py:38-61): every ball whose centre lies in neither goal triangle is a candidate; all (hive robot,
// candidate ball) pairs are sorted by MyUtils.distance of the two centres, ascending; the list is walked and a pair is taken when
// neither its robot nor its ball is taken yet.  The reference builds the list ball-major and iterates a Python set of players, so
// the order of exactly equal distances is not defined by it; here it is: ball index, then robot index (a stable sort with the hive
// iterated in robot order).  Distances are compared in the handle's arithmetic type.  With the opt-in goal scoring a consumed ball
// (out of play) is no candidate -- the reference removes it from lstBalls.
//
// Lane-loop style like rr_sim.hpp: the same source runs as SIMT code on the GPU and as lane loops under g++ (tests/emu/rr_hive_emu.cpp).
#pragma once
#include "rr_sim.hpp"
#include "rr_extras.hpp"

namespace rr {

// (distance, pair index) minimum over the lanes of a virtual wave, lexicographic; afterwards every lane holds the winner.
// Butterfly over the VW lanes of the group: the partners of a lane are lanes of its own arena, so they are active whenever it is.
#if RR_GPU
template <int VW, typename R> __device__ __forceinline__ void vw_argmin(R &d, int &p) {
#pragma unroll
    for (int off = VW / 2; off >= 1; off >>= 1) {
        const R od = __shfl_xor(d, off, VW);
        const int op = __shfl_xor(p, off, VW);
        if (od < d || (od == d && op < p)) { d = od; p = op; }
    }
}
#else
template <int VW, typename R> inline void vw_argmin(R (&d)[VW], int (&p)[VW]) {
    int w = 0;
    for (int l = 1; l < VW; l++) if (d[l] < d[w] || (d[l] == d[w] && p[l] < p[w])) w = l;
    const R wd = d[w];
    const int wp = p[w];
    for (int l = 0; l < VW; l++) { d[l] = wd; p[l] = wp; }
}
#endif

// The greedy assignment.  robot_mask: the hive (bit r = robot r, happy robots first).  got: bit r = robot r was given a ball;
// which: that ball's index in bits 4r .. 4r+3 (NB <= 16).  Both are uniform over the arena's lanes.
//   (a) one lane per ball: candidate? (ballot) ; one lane per (ball, robot) pair, pair = ball * NR + robot: the distance, in registers
//   (b) at most min(NR, NB) rounds: every lane's best free pair, arg-min across the lanes, the winner's robot and ball are taken
template <class C>
RR_HD void hive_assign(const Arena<C> &A, const SimParams<typename C::Real> &sp, uint32_t robot_mask, uint32_t &got, uint64_t &which) {
    using R = typename C::Real;
    constexpr int NP = C::NR * C::NB, KP = (NP + C::VW - 1) / C::VW; // pairs per lane
    constexpr int ROUNDS = C::NR < C::NB ? C::NR : C::NB;
    static_assert(C::NB <= 16 && C::NR <= 16, "a ball index per robot in four bits");
    struct PD { R d[KP]; };
    uint64_t bm = 0; // candidate balls
    RR_FOR_LANES(l) {
        bool cand = false;
        if (l < C::NB) {
            int st = 0;
            const V2<R> c = { A.p.bcx[l], A.p.bcy[l] };
            cand = ball_in_play(A, l) && !goal_contains<R>(false, sp.W, sp.H, c, st) && !goal_contains<R>(true, sp.W, sp.H, c, st);
        }
        RR_VOTE(bm, l, cand);
    }
    RR_LANE_VAR(PD, dl);
    RR_FOR_LANES(l) {
        for (int k = 0; k < KP; k++) {
            const int p = k * C::VW + l;
            R d = inf_<R>(); // not a pair of the list
            if (p < NP) {
                const int b = p / C::NR, r = p % C::NR;
                if (((bm >> b) & 1u) && ((robot_mask >> r) & 1u)) {
                    const V2<R> bc = { A.p.bcx[b], A.p.bcy[b] }, rc = { A.p.rcx[r], A.p.rcy[r] };
                    d = dist<R>(bc, rc);
                }
            }
            RR_LV(dl, l).d[k] = d;
        }
    }
    uint32_t rt = 0, bt = 0;
    uint64_t wh = 0;
    for (int round = 0; round < ROUNDS; round++) {
        RR_LANE_VAR(R, bd);
        RR_LANE_VAR(int, bp);
        RR_FOR_LANES(l) {
            R d = inf_<R>();
            int p = NP;
            for (int k = 0; k < KP; k++) { // ascending pair index: the first of equal distances stays
                const int pp = k * C::VW + l;
                if (pp < NP) {
                    const int b = pp / C::NR, r = pp % C::NR;
                    const R dd = RR_LV(dl, l).d[k];
                    if (!((rt >> r) & 1u) && !((bt >> b) & 1u) && dd < d) { d = dd; p = pp; }
                }
            }
            RR_LV(bd, l) = d;
            RR_LV(bp, l) = p;
        }
        vw_argmin<C::VW>(bd, bp);
        const int wp = RR_LV(bp, 0);
        if (wp >= NP) break; // no free pair left (uniform over the arena's lanes)
        const int b = wp / C::NR, r = wp % C::NR;
        rt |= 1u << r;
        bt |= 1u << b;
        wh |= (uint64_t)b << (4 * r);
    }
    got = rt;
    which = wh;
}

// Assignment + the observation of every hive robot with its own ball: assign [NR], obs [NR][11] of this arena.
// kind OBS_V2: the lane-parallel observe() once per assigned robot (A must be derive()d); OBS_V1: observe_kind, serial per robot, the
// robots spread over the arena's lanes (q = the arena's record).  Rows of robots without a ball are 0.
// (KIND is a template parameter: a kernel that holds both observers needs every register the file has.)
template <class C, typename O, int KIND>
RR_HD void hive_observe(Arena<C> &A, const Rec<C> &q, const SimParams<typename C::Real> &sp, uint32_t robot_mask, int32_t *assign,
                         O *obs) {
    uint32_t got;
    uint64_t which;
    hive_assign<C>(A, sp, robot_mask, got, which);
    RR_FOR_LANES(l) {
        if (l < C::NR) assign[l] = ((got >> l) & 1u) ? (int32_t)((which >> (4 * l)) & 15u) : -1;
    }
    if constexpr (KIND == OBS_V2) {
#pragma unroll 1
        for (int r = 0; r < C::NR; r++) { // (one copy of observe(): the robots' turns differ in indices only)
            if ((got >> r) & 1u) {
                int st = 0;
                observe<C, O>(A, sp, r < C::NRH ? 1 : -1, r, (int)((which >> (4 * r)) & 15u), obs + 11 * r, st);
            } else {
                for (int base = 0; base < 11; base += C::VW) { RR_FOR_LANES(l) { if (base + l < 11) obs[11 * r + base + l] = (O)0; } }
            }
        }
    } else {
        RR_FOR_LANES(l) {
            if (l < C::NR) {
                O *o = obs + 11 * l;
                if ((got >> l) & 1u) observe_kind<C, O>(q, sp, OBS_V1, l < C::NRH ? 1 : -1, l, (int)((which >> (4 * l)) & 15u), o);
                else for (int k = 0; k < 11; k++) o[k] = (O)0;
            }
        }
    }
}

// ---- training the hive in the full game: the transition of every hive robot over the step that was just taken.
//
// The reference has no per-robot reward; this is the project's definition: for robot r going for ball b, SimpleDuel3's three keepers
// restricted to that pair.  Starting from (R)0, in this order:
//   1. NaughtyBots:        -0.005 if bit 16 + r of the step's status is set;
//   2. ChasePosBall:       (dist(prior_r, ball_now) - dist(robot_now, ball_now)) * mult_robot -- prior_r the robot's on_step_begin copy
//                          (xs[3 r], xs[3 r + 1]), ball_now the ball's centre AFTER the step in both distances, as the reference has it;
//   3. PushPosBallsToGoal: sgn * (dist((0,0), ball_now) - dist((0,0), ball_prior)) * mult_ball -- ball_prior the snapshot's ball copy
//                          (xs_ball<C>(b)); sgn = (r happy ? +1 : -1) * (b positive ? +1 : -1): negative exactly for the pairs whose view
//                          observe() turns round (`flip`), so a policy trained in preset T sees one consistent game.
// `dist` here is ref_dist below -- MyUtils.distance as the reference evaluates it, ((bx - ax) ** 2 + (by - ay) ** 2) ** .5 with both
// powers through libm's pow -- NOT the step kernel's dist<R> (x * x and sqrt, a last-bit difference on about one distance in a thousand).
// With one robot per team and positive ball 0 the sum is then the REFERENCE's team reward bit for bit on the host, on every recorded step
// of presets T and D (tests/test_hive_transition_emulated.py; with dist<R> 6 of T's 4,564 steps are off by up to 2.7e-11).  On the device
// pow is the device library's: equal to k_step's reward and to the reference's within a few 1e-11 (tests/test_gpu_hive_transition.py: 1e-9).
// The cost is five pow-based distances per hive robot and launch, next to an 11-value lidar observation.
//
// A row is VALID when its robot is in robot_mask, 0 <= assign[r] < NB (any other value is never used as an index), the step's status
// has none of WAS_RESET / NOT_READY / STEP_AFTER_DONE, and the ball is still in play (with the opt-in goal scoring a ball consumed
// during this step ends the pairing without a transition).  next_obs of a valid row is the robot's observation of THE SAME ball on the
// record after the step -- the ball is held, not re-assigned, even if it now lies in a goal.  Invalid rows are all 0.
// assign [NR], next_obs [NR][11], reward / terminal / valid [NR] of this arena; xs the arena's on_step_begin snapshot (rr_extras.hpp).
// Kind as in hive_observe (kind OBS_V2: A must be derive()d).  Read-only on A's persistent part, q and xs; no atomics.
RR_HD double m_pow(double x, double y) { return ::pow(x, y); }
RR_HD float m_pow(float x, float y) { return ::powf(x, y); }
template <typename R> RR_HD R ref_dist(V2<R> a, V2<R> b) { // MyUtils.py:40-41, `**` as CPython evaluates it
    return m_pow(m_pow(b.x - a.x, (R)2) + m_pow(b.y - a.y, (R)2), (R).5);
}
template <class C, typename O, int KIND>
RR_HD void hive_transition(Arena<C> &A, const Rec<C> &q, const SimParams<typename C::Real> &sp, const typename C::Real *xs,
                            uint32_t robot_mask, const int32_t *assign, int32_t status, uint8_t done, O *next_obs, O *reward,
                            uint8_t *terminal, uint8_t *valid) {
    using R = typename C::Real;
    static_assert(C::NB <= 16 && C::NR <= 16, "a ball index per robot in four bits, a NaughtyBots bit per robot in status bits 16..31");
    const bool stepped = !(status & (ST_WAS_RESET | ST_NOT_READY | ST_STEP_AFTER_DONE));
    uint32_t ok = 0;     // bit r = row r is valid; uniform over the arena's lanes (every lane reads the arena's NR words)
    uint64_t which = 0;  // its ball in bits 4r .. 4r+3
    for (int r = 0; r < C::NR; r++) {
        const int32_t b = assign[r];
        if (stepped && ((robot_mask >> r) & 1u) && b >= 0 && b < C::NB && ball_in_play(A, b)) {
            ok |= 1u << r;
            which |= (uint64_t)b << (4 * r);
        }
    }
    // rewards: one lane per robot, the snapshot words and the record's centres straight from HBM
    RR_FOR_LANES(l) {
        if (l < C::NR) {
            R rw = (R)0;
            const bool v = (ok >> l) & 1u;
            if (v) {
                const int b = (int)((which >> (4 * l)) & 15u);
                if (((uint32_t)status >> (16 + l)) & 1u) rw -= (R).005;
                const V2<R> bc = { q.bcx(b), q.bcy(b) }, rc = { q.rcx(l), q.rcy(l) }, pc = { xs[3 * l], xs[3 * l + 1] };
                rw += (ref_dist<R>(pc, bc) - ref_dist<R>(rc, bc)) * sp.mult_robot;
                const V2<R> o = { (R)0, (R)0 }, pb = { xs[xs_ball<C>(b)], xs[xs_ball<C>(b) + 1] };
                const R push = (ref_dist<R>(o, bc) - ref_dist<R>(o, pb)) * sp.mult_ball;
                const bool flip = (l < C::NRH) != (b < C::NBP);
                if (flip) rw -= push; else rw += push;
            }
            reward[l] = (O)rw;
            terminal[l] = v ? done : (uint8_t)0;
            valid[l] = v ? 1 : 0;
        }
    }
    if constexpr (KIND == OBS_V2) {
#pragma unroll 1
        for (int r = 0; r < C::NR; r++) { // (one copy of observe(), as in hive_observe)
            if ((ok >> r) & 1u) {
                int st = 0;
                observe<C, O>(A, sp, r < C::NRH ? 1 : -1, r, (int)((which >> (4 * r)) & 15u), next_obs + 11 * r, st);
            } else {
                for (int base = 0; base < 11; base += C::VW) { RR_FOR_LANES(l) { if (base + l < 11) next_obs[11 * r + base + l] = (O)0; } }
            }
        }
    } else {
        RR_FOR_LANES(l) {
            if (l < C::NR) {
                O *o = next_obs + 11 * l;
                if ((ok >> l) & 1u) observe_kind<C, O>(q, sp, OBS_V1, l < C::NRH ? 1 : -1, l, (int)((which >> (4 * l)) & 15u), o);
                else for (int k = 0; k < 11; k++) o[k] = (O)0;
            }
        }
    }
}

// ---- the hive under the budgeted step: held rows.
//
// Under a step budget an arena's step may span several calls (rr_sim.hpp: park_save).  While it is parked its record holds the middle
// of that step, and the step ignores whatever thrust it is given.  The transition the arena completes later belongs to the assignment
// it was given, the observation the agent was asked on and the action it answered BEFORE the step began -- so those three rows are held
// while the arena is parked: hive_hold() keeps the observer off them, hive_commit() keeps the agent's fresh (wasted) answer out of them,
// and hive_idle() writes the "no transition yet" row without touching the record.  The parked mark is read from the record
// (record_parked), not from a caller's status: whatever rewrites an arena from outside clears it, and the arena is observed afresh.

// held[0] = the arena is parked mid-step (irec: the int part of its record); true: the caller leaves the arena's assign / obs rows alone
template <class C> RR_HD bool hive_hold(const int32_t *irec, uint8_t *held) {
    const bool parked = record_parked<C>(irec); // (uniform over the arena's lanes: one word of its record)
    RR_FOR_LANES(l) { if (l == 0) held[0] = parked ? 1 : 0; }
    return parked;
}

// GameEnv_Simple._dct_thrust_from_direction (RR_EnvBase.py:593-602): Direction 0..7 -> (L, R); anything else is no direction: (0, 0)
RR_HD void thrust_from_direction(int32_t dir, float &tl, float &tr) {
    const float t[8][2] = { { 1.f, 1.f }, { -1.f, -1.f }, { -1.f, 1.f }, { 1.f, -1.f }, { 0.f, 1.f }, { 1.f, 0.f }, { -1.f, 0.f }, { 0.f, -1.f } };
    const bool ok = dir >= 0 && dir < 8;
    const int k = ok ? dir : 0; // (an out-of-range value is never an index)
    tl = ok ? t[k][0] : 0.f;
    tr = ok ? t[k][1] : 0.f;
}

// The tail of the hive's turn for ONE (arena, robot) cell -- no record needed: the agent's fresh answer is accepted unless the arena is
// held.  fresh / assign / accepted [NR] and thrust [2 NR] of the arena, held its byte.  A held arena and a robot outside the mask keep
// their accepted action and their thrust pair (another player drives the latter); a robot without a ball stands still.
RR_HD void hive_commit(uint32_t robot_mask, int r, const int32_t *fresh, const int32_t *assign, uint8_t held, int32_t *accepted,
                       float *thrust) {
    if (held || !((robot_mask >> r) & 1u)) return;
    const int32_t f = fresh[r];
    accepted[r] = f;
    float tl, tr;
    thrust_from_direction(assign[r] >= 0 ? f : -1, tl, tr);
    thrust[2 * r] = tl;
    thrust[2 * r + 1] = tr;
}

// An arena whose status says it did not step (re-placed, parked, stepped after done) has no transition: the rows hive_transition
// writes for it -- all 0 -- without its record.  false: the arena stepped, nothing was written.
template <class C, typename O>
RR_HD bool hive_idle(int32_t status, O *next_obs, O *reward, uint8_t *terminal, uint8_t *valid) {
    if (!(status & (ST_WAS_RESET | ST_NOT_READY | ST_STEP_AFTER_DONE))) return false;
    for (int base = 0; base < 11 * C::NR; base += C::VW) { RR_FOR_LANES(l) { if (base + l < 11 * C::NR) next_obs[base + l] = (O)0; } }
    RR_FOR_LANES(l) {
        if (l < C::NR) { reward[l] = (O)0; terminal[l] = 0; valid[l] = 0; }
    }
    return true;
}

} // namespace rr
