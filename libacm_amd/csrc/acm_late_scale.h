/*
 * acm_late_scale.h - the power of two that level 9 takes into its cascade in the LAST LDS pass instead of at the unpack.
 *
 * OutScale (acm_kernels.hip) scales the whole cascade at the unpack so that the 16 sample bits end on a byte boundary and one
 * v_perm_b32 packs a pair.  Level 9 cannot: it needs bits 9..24, and the one-op v_mad_i32_i24 butterfly keeps 25 bits.  But the
 * cascade is linear mod 2^32, so the scale may enter at any stage, and in a last pass of G >= 2 stages it enters for nothing:
 *   stage G-2 (stage 7, kind P) multiplies by 2^7 through the shift operands its two instructions have anyway.  Its inputs are
 *             exact in bits [0, 25), its outputs therefore in all 32;
 *   stage G-1 (stage 8, kind N) runs on the scaled values with the exact two-op forms (no 24-bit multiply);
 *   the sample, bits [9, 25) of the plain result, sits in bits [16, 32) = bytes 2..3, as at levels >= 10.
 * Histories and the carry buffer hold each stage's INPUTS, so the last stage's history is in scaled units on both sides of a chunk
 * or tile boundary (the warm-up body runs the same forms), and zeros stay zeros.
 *
 * No HIP header.  In a device pass each form below is ONE asm statement of two instructions: opaque, as add_twice / sub_twice are, so
 * that the compiler neither re-associates the butterfly nor falls back to v_mul_lo_u32; and one statement, because the compiler puts
 * an s_nop in front of an asm statement that reads what another one wrote with no instruction of its own in between, and an s_nop
 * costs an issue slot like any instruction (profiles/level9_byte_writeout_notes.txt 1).  Anywhere else they are the same expressions
 * in plain C++ (tests/native/late_scale.cpp drives those).
 */
#ifndef ACM_LATE_SCALE_H
#define ACM_LATE_SCALE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define ACM_LATE_FN __host__ __device__ __forceinline__
#else
#define ACM_LATE_FN static inline
#endif

namespace acm_late {

/* a LAST pass of G stages at level L */
template <int L, int G>
struct LateScale {
	static constexpr bool ON = (L == 9 && G >= 2);          /* a last pass of one stage (tuning groupings only) has no P stage to take the scale */
	static constexpr int INJECT = ON ? G - 2 : -1;          /* stage of the pass (kind P) that multiplies by 2^SHIFT */
	static constexpr int EXACT = ON ? G - 1 : -1;           /* stage of the pass (kind N) that runs exact mod 2^32 */
	static constexpr int SHIFT = ON ? 16 - L : 0;
	static constexpr int BYTE = 2;                          /* first byte of the sample inside the value (ON only) */
};

constexpr int SHIFT9 = LateScale<9, 3>::SHIFT;
static_assert(SHIFT9 == 7, "the injecting forms below are written for 2^7");

/* v_mad_i32_i24 d, a, b, c: the low 24 bits of a and b as signed numbers, d = a * b + c mod 2^32 */
ACM_LATE_FN uint32_t mad_i24(uint32_t a, int32_t b, uint32_t c)
{
	const int32_t a24 = (int32_t)(a << 8) >> 8, b24 = (int32_t)((uint32_t)b << 8) >> 8;
	return (uint32_t)((int64_t)a24 * b24) + c;
}

/* kind P, even position, times 128: (z2 + z0 + 2 z1) << 7 */
ACM_LATE_FN uint32_t p_inject_even(uint32_t z0, uint32_t z1, uint32_t z2)
{
#if defined(__HIP_DEVICE_COMPILE__)
	uint32_t y;
	asm("v_add_lshl_u32 %0, %1, %2, 7\n\tv_lshl_add_u32 %0, %3, 8, %0" : "=&v"(y) : "v"(z2), "v"(z0), "v"(z1));
	return y;
#else
	const uint32_t t = (z2 + z0) << SHIFT9;
	return (z1 << (SHIFT9 + 1)) + t;
#endif
}

/* kind P, odd position (stored negated), times 128: (z2 + z0 - 2 z1) << 7.  The multiply reads z1[23:0] as a signed number; what it
 * leaves out is a multiple of 2^24, times 256 = 0 mod 2^32 */
ACM_LATE_FN uint32_t p_inject_odd(uint32_t z0, uint32_t z1, uint32_t z2)
{
#if defined(__HIP_DEVICE_COMPILE__)
	uint32_t y;
	asm("v_add_lshl_u32 %0, %1, %2, 7\n\tv_mad_i32_i24 %0, %3, %4, %0"              /* (no literal in a VOP3: the -256 is a scalar register) */
	    : "=&v"(y) : "v"(z2), "v"(z0), "v"(z1), "s"(-(2 << SHIFT9)));
	return y;
#else
	const uint32_t t = (z2 + z0) << SHIFT9;
	return mad_i24(z1, -(2 << SHIFT9), t);
#endif
}

/* kind N, exact mod 2^32: (z0 - z2) - 2 z1 = z0 - (2 z1 + z2) */
ACM_LATE_FN uint32_t n_exact_sub(uint32_t z0, uint32_t z1, uint32_t z2)
{
#if defined(__HIP_DEVICE_COMPILE__)
	uint32_t y;
	asm("v_lshl_add_u32 %0, %1, 1, %2\n\tv_sub_u32 %0, %3, %0" : "=&v"(y) : "v"(z1), "v"(z2), "v"(z0));
	return y;
#else
	const uint32_t t = (z1 << 1) + z2;
	return z0 - t;
#endif
}

/* kind N, exact mod 2^32: (z2 - z0) + 2 z1 */
ACM_LATE_FN uint32_t n_exact_add(uint32_t z0, uint32_t z1, uint32_t z2)
{
#if defined(__HIP_DEVICE_COMPILE__)
	uint32_t y;
	asm("v_sub_u32 %0, %1, %2\n\tv_lshl_add_u32 %0, %3, 1, %0" : "=&v"(y) : "v"(z2), "v"(z0), "v"(z1));
	return y;
#else
	const uint32_t t = z2 - z0;
	return (z1 << 1) + t;
#endif
}

/* v_perm_b32(S0 = second value, S1 = first value, selector): byte k of S1 is index k, of S0 index 4 + k.  The selector that packs the
 * samples at bytes lo, lo + 1 of two values into one dword, first sample in the low half, each byte-swapped if asked */
ACM_LATE_FN uint32_t perm_sel(uint32_t lo, bool be)
{
	const uint32_t hi = lo + 1;
	return be ? ((4 + lo) << 24 | (4 + hi) << 16 | lo << 8 | hi)
		  : ((4 + hi) << 24 | (4 + lo) << 16 | hi << 8 | lo);
}

/* the xor that turns a packed pair of signed samples into unsigned ones */
ACM_LATE_FN uint32_t perm_flip(bool be, bool uns)
{
	return uns ? (be ? 0x00800080u : 0x80008000u) : 0u;
}

}  // namespace acm_late

#endif
