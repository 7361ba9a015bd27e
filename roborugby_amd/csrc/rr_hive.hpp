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

} // namespace rr
