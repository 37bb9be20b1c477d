/*
 * acm_kernels_f32.hip - the float32 builds of the synthesis kernels (acmhip_plan_launch_f32): acm_kernels.hip once more, with
 * ACM_OUT_F32 = 1, as a translation unit of its own (see the comment on ACM_OUT_F32 there for why).  Each kernel writes the
 * ACMHIP_FMT_S16LE sample times 2^-15 from the same parked int16 pairs; the launchers carry an _f32 suffix and are reached through
 * fmt | ACMK_FMT_F32 of the int16 ones.
 */
#define ACM_OUT_F32 1
#include "acm_kernels.hip"
