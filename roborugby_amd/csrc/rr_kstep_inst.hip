// rr_kstep_inst.hip -- explicit instantiations of the step kernel for one share (-DRR_PART=k, k < RR_KSTEP_PARTS) of the built
// configurations: the product build compiles the shares in parallel (roborugby_amd/build.py); see rr_kstep.hpp.
#include "rr_kstep.hpp"

#ifndef RR_PART
#error "compile with -DRR_PART=<0..RR_KSTEP_PARTS-1>"
#endif
#define RR_NOTHING
// (a macro cannot compare its argument with RR_PART, so every row expands to a constexpr-guarded nothing or to its instantiations
// through a second macro level keyed on the row's own part number)
#define RR_IF_PART_0(...)
#define RR_IF_PART_1(...)
#define RR_IF_PART_2(...)
#define RR_IF_PART_3(...)
#if RR_PART == 0
#undef RR_IF_PART_0
#define RR_IF_PART_0(...) __VA_ARGS__
#elif RR_PART == 1
#undef RR_IF_PART_1
#define RR_IF_PART_1(...) __VA_ARGS__
#elif RR_PART == 2
#undef RR_IF_PART_2
#define RR_IF_PART_2(...) __VA_ARGS__
#elif RR_PART == 3
#undef RR_IF_PART_3
#define RR_IF_PART_3(...) __VA_ARGS__
#else
#error "RR_PART out of range"
#endif

#define X(kind_, part_, a, b, c, d, R_, vw_) RR_IF_PART_##part_(RR_KSTEP_INST_##R_(RR_NOTHING, a, b, c, d, vw_))
RR_CFG_TABLE(X)
#undef X
