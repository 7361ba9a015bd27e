// rr_kstep.hpp -- the step kernel template (k_step) and the table of built configurations.
//
// Shared by rr_kernels.hip (the C-ABI + every other kernel) and rr_kstep_inst.hip: the product build compiles the k_step
// instantiations -- nine configurations x up to five variants, most of the library's compile time -- in parallel translation
// units (rr_kstep_inst.hip with -DRR_PART=k holds the explicit instantiations of its share, rr_kernels.hip declares them
// `extern template` under -DRR_SPLIT_BUILD).  No relocatable device code is involved: every kernel is self-contained, each
// object registers its own code object, the host side only needs the launch stubs at link time.  Tuning builds
// (tools/build_variant.sh, tools/kernel_resources.py) keep the single translation unit with implicit instantiation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "rr_sim.hpp"

using namespace rr;

// ------------------------------------------------------------------------------------------------ device side
// (under the F32State policy `rec` holds fp32 values: they are widened on the way into LDS and rounded once on the way back)
template <class C> __device__ __forceinline__ void load_record(Arena<C> &A, const typename C::Store *rec, const int32_t *irec) {
    using R = typename C::Real;
    R *p = reinterpret_cast<R *>(&A.p);
    int32_t *q = reinterpret_cast<int32_t *>(&A.i);
    const int lane = threadIdx.x & (C::VW - 1);
    for (int k = lane; k < Arena<C>::P_REALS; k += C::VW) p[k] = (R)rec[k];
    for (int k = lane; k < Arena<C>::I_INTS; k += C::VW) q[k] = irec[k];
    RR_SYNC();
}
template <class C> __device__ __forceinline__ void store_record(const Arena<C> &A, typename C::Store *rec, int32_t *irec) {
    using R = typename C::Real;
    const R *p = reinterpret_cast<const R *>(&A.p);
    const int32_t *q = reinterpret_cast<const int32_t *>(&A.i);
    const int lane = threadIdx.x & (C::VW - 1);
    RR_SYNC();
    for (int k = lane; k < Arena<C>::P_REALS; k += C::VW) rec[k] = (typename C::Store)p[k];
    // the ints and the record's padding: the whole 64-B tail is written, so no line of the record is left partially
    // dirty (a partial line costs a read-for-merge in L2: 0.3 KB per env-step showed up in FETCH_SIZE)
    constexpr int TAIL = Arena<C>::I_STRIDE - Arena<C>::P_REALS * Arena<C>::WS;
    for (int k = lane; k < TAIL; k += C::VW) irec[k] = k < Arena<C>::I_INTS ? q[k] : 0;
}

#ifndef RR_MIN_WAVES_PER_SIMD
#define RR_MIN_WAVES_PER_SIMD 4 // upper bound of the occupancy asked from the register allocator (<=128 VGPRs)
#endif
#ifndef RR_WAVES_PER_BLOCK
#define RR_WAVES_PER_BLOCK 1 // arenas never cooperate across wavefronts, so a workgroup IS a wavefront (finer dispatch: +9 % measured)
#endif
constexpr int WAVES_PER_BLOCK = RR_WAVES_PER_BLOCK;
template <class C> constexpr int arenas_per_block() { return 64 * WAVES_PER_BLOCK / C::VW; }
// Waves per SIMD the 160 KiB of LDS admit for this configuration.  Asking the register allocator for more than that
// (launch bounds) only buys spills: with 17 KB of LDS per wavefront G/VW=8 and T/VW=2 top out at 2 waves/SIMD, and
// capping them at 128 VGPRs put ~30 scratch round trips into every sub-step (measured: 487 VMEM instructions per
// wave-step instead of ~90, and a 0.25 ms latency floor per launch).
template <class C> constexpr int lds_waves_per_simd() {
    constexpr int per_cu = (160 * 1024) / (int)(sizeof(Arena<C>) * arenas_per_block<C>()) * WAVES_PER_BLOCK;
    return per_cu / 4 < 1 ? 1 : (per_cu / 4 > RR_MIN_WAVES_PER_SIMD ? RR_MIN_WAVES_PER_SIMD : per_cu / 4);
}


// MULTI = false: rr_step, one step per launch (nsteps, repeat unused); true: rr_rollout's loop over nsteps.  Separate
// instantiations: the loop around step_arena costs the single-step kernel 12 % (measured) through register allocation alone.
// BUDGET = true: the budgeted step (rr_sim.hpp: ParkCtx) -- a separate instantiation, so the default kernel carries none of it.
template <class C, typename O, bool MULTI, bool BUDGET = false>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, lds_waves_per_simd<C>()) void k_step(SimParams<typename C::Real> sp, typename C::Store *recs,
                                                              int32_t *irecs, int n, const int32_t *actions,
                                                              const float *thrust, int na, O *obs, O *reward,
                                                              uint8_t *done, O *obs_g, O *reward_g, int32_t *status,
                                                              const uint32_t *order, uint32_t *cost, int nsteps, int repeat,
                                                              uint32_t *snap, int32_t *isnap, uint32_t *park = nullptr,
                                                              uint32_t budget = 0) {
    static_assert(!(MULTI && BUDGET), "rr_rollout keeps the record in LDS across steps: no barrier to budget");
    __shared__ Arena<C> lds[arenas_per_block<C>()];
    const int wave = threadIdx.x / C::VW; // virtual wave = arena slot in this workgroup
    // slowest-first dispatch: workgroup b steps the group of arenas that was the b-th slowest in the previous step
    const unsigned long long t_begin = (cost || BUDGET) ? __builtin_amdgcn_s_memtime() : 0ull;
    const int group = order ? (int)order[blockIdx.x] : (int)blockIdx.x;
    const int arena = group * arenas_per_block<C>() + wave;
    if (arena >= n) return; // uniform per virtual wave; no workgroup barrier is ever used
    Arena<C> &A = lds[wave];
    typename C::Store *rec = recs + (size_t)arena * Arena<C>::P_STRIDE;
    int32_t *irec = irecs + (size_t)arena * Arena<C>::I_STRIDE;
    RR_T0();
#if defined(RR_PROFILE_PHASES)
    const unsigned long long rr_wave_t0_ = __builtin_amdgcn_s_memrealtime(); // 100 MHz, one base for the whole chip
#endif
    load_record(A, rec, irec);
    derive(A, sp);
    RR_STAMP(12);
    // The constants the sub-step loop reads (wall tests, corner renormalisation, the balls' inner rect) live in VECTOR registers.
    // As kernel arguments they are scalar values, loaded eight dwords at a time together with the reward multipliers, and the loop has
    // no scalar registers left for them: the allocator parks them in lanes of a VGPR and every use in the loop reads the whole group
    // back (v_readlane + hazard slots: 48 of the 114 lane reads in the loop's head run, tools/loop_spill_traffic.py).  Only where
    // vector registers are to spare: the single-step kernels with fp64 arithmetic (G 241 of 256, no spills in any of their rows).  The
    // budgeted and the multi-step kernels sit at 256, and the all-fp32 rows are capped at 168 / 128 VGPRs by their launch bounds and
    // already spill (five more pinned registers only added scratch traffic there): those keep the arguments as they are.
    // Uniform values in vector registers: same operands, same operations, same results.
    SimParams<typename C::Real> sph = sp;
    if constexpr (!MULTI && !BUDGET && sizeof(typename C::Real) == 8) {
        asm volatile("" : "+v"(sph.W), "+v"(sph.H), "+v"(sph.rob_cdist));
        asm volatile("" : "+v"(sph.inner_h), "+v"(sph.inner_cdist));
    }
    // The robot move's tail runs on both lanes of the robot's pair, by component (rr_sim.hpp: robot_move_comp_begin), except where that
    // loses: the all-fp32 rows capped at 128 VGPRs by four waves per SIMD (D) spill already, and their budgeted and multi-step kernels,
    // which carry the park state / the loop over the steps on top, spill 57 -> 96 and 78 -> 88 VGPRs with it and measured -2.9 % and
    // -2.7 % (profiles/pair_move/).  Those keep the tail on one lane; every other row gains 1-6 %.  Same results either way.
    constexpr bool COMP = !((MULTI || BUDGET) && sizeof(typename C::Real) == 4 && lds_waves_per_simd<C>() >= 4);
    if constexpr (!MULTI) {
        StepOut<O> o = { obs, obs_g, reward, reward_g, done, status, sp.memo ? snap : nullptr, isnap, arena,
                         (int)Arena<C>::SNAP_WORDS, (int)Arena<C>::ISNAP_WORDS };
        if constexpr (BUDGET) {
            ParkCtx pk;
            pk.buf = park + (size_t)arena * Arena<C>::PARK_WORDS; pk.budget = budget; pk.t_begin = t_begin;
            step_arena<C, O, true, COMP>(A, sph, sp.arena_offset + (uint64_t)arena, actions ? actions + (size_t)arena * na : nullptr,
                                   thrust ? thrust + (size_t)arena * 2 * na : nullptr, na, o, pk);
        } else {
            step_arena<C, O, false, COMP>(A, sph, sp.arena_offset + (uint64_t)arena, actions ? actions + (size_t)arena * na : nullptr,
                             thrust ? thrust + (size_t)arena * 2 * na : nullptr, na, o);
        }
    } else {
        // nsteps consecutive GameEnv.step calls on the record held in LDS (rr_rollout): step s reads its actions at
        // [s][arena] (or the same ones again when `repeat`) and writes its outputs at [s][arena]
#pragma unroll 1
        for (int s = 0; s < nsteps; s++) {
            const size_t so = (size_t)s * (size_t)n;
            StepOut<O> o = { obs + so * 11, obs_g ? obs_g + so * 11 : nullptr, reward + so, reward_g ? reward_g + so : nullptr, done + so,
                             status ? status + so : nullptr, sp.memo ? snap : nullptr, isnap, arena,
                             (int)Arena<C>::SNAP_WORDS, (int)Arena<C>::ISNAP_WORDS };
            const size_t ao = repeat ? 0 : so;
            step_arena<C, O, false, COMP>(A, sph, sp.arena_offset + (uint64_t)arena, actions ? actions + (ao + (size_t)arena) * na : nullptr,
                             thrust ? thrust + (ao + (size_t)arena) * 2 * na : nullptr, na, o);
        }
    }
    RR_TR();
    {   // the record addresses again, from an arena index the optimiser cannot tie to the first one: otherwise the two
        // 64-bit pointers stay live across the whole step (4 VGPRs of a kernel that sits at the 256-VGPR limit)
        int arena_again = arena;
        asm volatile("" : "+v"(arena_again));
        store_record(A, recs + (size_t)arena_again * Arena<C>::P_STRIDE, irecs + (size_t)arena_again * Arena<C>::I_STRIDE);
    }
    RR_STAMP(13);
    if (cost && threadIdx.x == 0) { // what this group cost, in shader clocks / 256 (saturating): next step's dispatch key
        const unsigned long long dt = ((__builtin_amdgcn_s_memtime() - t_begin) >> 8) / (unsigned)(MULTI ? nsteps : 1); // per step
        cost[group] = dt > 0xFFFFull ? 0xFFFFu : (uint32_t)dt;
    }
#if defined(RR_PROFILE_PHASES)
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 65536) {
        g_rr_wave_t[2 * blockIdx.x] = rr_wave_t0_;
        g_rr_wave_t[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
    }
#endif
}

// Built configurations, one row each: X(kind, part, NRH, NRG, NBP, NBN, precision, VW)
//   kind      = shape + RR_NUM_SHAPES * dtype -- shapes: 0 = T (1+0 robots, 1+0 balls), 1 = G (2+2, 4+4), 2 = D (1+1, 1+1: the two-team duel);
//               dtype 0: fp64, 1: fp32, 2: fp32 state with fp64 arithmetic (rr_sim.hpp: F32State)
//   part      = the translation unit of the split build (rr_kstep_inst.hip -DRR_PART=part) that holds the row's k_step instantiations:
//               no two G rows share a part (the G and D kernels are the slow ones to compile); the parts are balanced so that each
//               compiles in less time than rr_kernels.hip itself, which bounds the build (measured at 8 jobs: profiles/one_width/)
//   precision = double | float | F32State; it also decides which k_step variants exist (RR_KSTEP_INST_<precision> below)
//   VW        = lanes per arena: one width per kind (T 2, G 8, D 4), the one every handle of that kind gets.  Other widths are
//               measured with tuning builds (RR_TUNE_VW_* below), never carried by the product library
// Everything else -- dispatch, the shapes rr_create recognises, the extern declarations and the explicit instantiations of the split
// build, roborugby_amd/build.py's KSTEP_PARTS and BUILT_SHAPES -- is derived from these rows.
#define RR_KSTEP_PARTS 4
#if defined(RR_CUSTOM_SHAPE)
// A library for ONE shape outside the built list (roborugby_amd.build.build_shape_library: the reference's entity counts are free
// integers, RR_Constants.py:30-34): -DRR_CUSTOM_SHAPE -DRR_NRH= -DRR_NRG= -DRR_NBP= -DRR_NBN= -DRR_CVW=<lanes per arena> (+ RR_CFG_SUBSET:
// one translation unit, implicit instantiation).  Precisions: fp64 and fp32 state / fp64 arithmetic.
#define RR_CFG_TABLE(X) X(0, 0, RR_NRH, RR_NRG, RR_NBP, RR_NBN, double, RR_CVW) X(6, 0, RR_NRH, RR_NRG, RR_NBP, RR_NBN, F32State, RR_CVW)
#elif defined(RR_CFG_SUBSET)
// Tuning builds only (tools/build_variant.sh, tools/kernel_resources.py): T and G in fp64, quick to compile, at -DRR_TUNE_VW_T=<lanes> /
// -DRR_TUNE_VW_G=<lanes> per arena (default: the product's widths); -DRR_TUNE_VW_D=<lanes> adds the duel shape (the product's: 4).
#ifndef RR_TUNE_VW_T
#define RR_TUNE_VW_T 2
#endif
#ifndef RR_TUNE_VW_G
#define RR_TUNE_VW_G 8
#endif
#ifdef RR_TUNE_VW_D
#define RR_TUNE_ROW_D(X) X(2, 0, 1, 1, 1, 1, double, RR_TUNE_VW_D)
#else
#define RR_TUNE_ROW_D(X)
#endif
#define RR_CFG_TABLE(X) X(0, 0, 1, 0, 1, 0, double, RR_TUNE_VW_T) X(1, 0, 2, 2, 4, 4, double, RR_TUNE_VW_G) RR_TUNE_ROW_D(X)
#else // the product library (roborugby_amd/build.py reads the rows between this line and the #endif)
#define RR_CFG_TABLE(X)                                                                                                 \
    X(0, 1, 1, 0, 1, 0, double, 2) X(1, 0, 2, 2, 4, 4, double, 8) X(2, 3, 1, 1, 1, 1, double, 4)                         \
    X(3, 0, 1, 0, 1, 0, float, 2) X(4, 1, 2, 2, 4, 4, float, 8) X(5, 2, 1, 1, 1, 1, float, 4)                            \
    X(6, 3, 1, 0, 1, 0, F32State, 2) X(7, 2, 2, 2, 4, 4, F32State, 8) X(8, 2, 1, 1, 1, 1, F32State, 4)
#endif
constexpr int RR_NUM_SHAPES = 3;
#define X(kind_, part_, a, b, c, d, R_, vw_) static_assert(part_ >= 0 && part_ < RR_KSTEP_PARTS && kind_ >= 0 && kind_ < 3 * RR_NUM_SHAPES, "row");
RR_CFG_TABLE(X)
#undef X

// ---- the k_step instantiations of a row: PREFIX = `extern` declares them (rr_kernels.hip under -DRR_SPLIT_BUILD: they live in
// rr_kstep_inst.hip's objects), empty defines them (rr_kstep_inst.hip).  Exactly what step_impl can launch for the row:
//   double  : plain + budgeted for float and double outputs, and rr_rollout's multi-step loop for float outputs
//   float   : plain + budgeted + multi-step, float outputs only
//   F32State: the plain single-step kernel only, float and double outputs
#define RR_KSTEP_SIG(C_, O_)                                                                                                       \
    (SimParams<typename C_::Real>, typename C_::Store *, int32_t *, int, const int32_t *, const float *, int, O_ *, O_ *, uint8_t *, \
     O_ *, O_ *, int32_t *, const uint32_t *, uint32_t *, int, int, uint32_t *, int32_t *, uint32_t *, uint32_t)
#define RR_KSTEP_CFG(a, b, c, d, R_, vw_) Cfg<a, b, c, d, R_, vw_>
#define RR_KSTEP_ONE(PREFIX, a, b, c, d, R_, vw_, O_, MULTI_, BUDGET_) \
    PREFIX template __global__ void k_step<Cfg<a, b, c, d, R_, vw_>, O_, MULTI_, BUDGET_> RR_KSTEP_SIG(RR_KSTEP_CFG(a, b, c, d, R_, vw_), O_);
#define RR_KSTEP_PLAIN(PREFIX, a, b, c, d, R_, vw_, O_) RR_KSTEP_ONE(PREFIX, a, b, c, d, R_, vw_, O_, false, false)
#define RR_KSTEP_BUDGET(PREFIX, a, b, c, d, R_, vw_, O_) RR_KSTEP_ONE(PREFIX, a, b, c, d, R_, vw_, O_, false, true)
#define RR_KSTEP_MULTI(PREFIX, a, b, c, d, R_, vw_, O_) RR_KSTEP_ONE(PREFIX, a, b, c, d, R_, vw_, O_, true, false)
#define RR_KSTEP_INST_double(PREFIX, a, b, c, d, vw_)                                                                                   \
    RR_KSTEP_PLAIN(PREFIX, a, b, c, d, double, vw_, float) RR_KSTEP_BUDGET(PREFIX, a, b, c, d, double, vw_, float)                      \
    RR_KSTEP_MULTI(PREFIX, a, b, c, d, double, vw_, float)                                                                              \
    RR_KSTEP_PLAIN(PREFIX, a, b, c, d, double, vw_, double) RR_KSTEP_BUDGET(PREFIX, a, b, c, d, double, vw_, double)
#define RR_KSTEP_INST_float(PREFIX, a, b, c, d, vw_)                                                                                    \
    RR_KSTEP_PLAIN(PREFIX, a, b, c, d, float, vw_, float) RR_KSTEP_BUDGET(PREFIX, a, b, c, d, float, vw_, float)                        \
    RR_KSTEP_MULTI(PREFIX, a, b, c, d, float, vw_, float)
#define RR_KSTEP_INST_F32State(PREFIX, a, b, c, d, vw_) \
    RR_KSTEP_PLAIN(PREFIX, a, b, c, d, F32State, vw_, float) RR_KSTEP_PLAIN(PREFIX, a, b, c, d, F32State, vw_, double)

#if defined(RR_SPLIT_BUILD) && !defined(RR_CFG_SUBSET)
#define X(kind_, part_, a, b, c, d, R_, vw_) RR_KSTEP_INST_##R_(extern, a, b, c, d, vw_)
RR_CFG_TABLE(X)
#undef X
#endif
