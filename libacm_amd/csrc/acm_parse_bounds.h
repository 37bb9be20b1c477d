/*
 * acm_parse_bounds.h - where the device parser's stripes and block ranges are cut.  One text for both readers: the kernels of
 * acm_parse.hip and the host's layouts (acmk_stripe_bound / acmk_range_bound, acm_kernel_geo.cpp).
 */
#ifndef ACM_PARSE_BOUNDS_H
#define ACM_PARSE_BOUNDS_H

#include <stdint.h>

#ifdef __HIP__          /* (any HIP compilation, with or without hip_runtime.h in front) */
#define ACM_BOUNDS_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define ACM_BOUNDS_FN static inline
#endif

/* striped upload: stripe s of S of a file's arena slot (the file, padded to 16 bytes, + 16 zero bytes) starts here */
ACM_BOUNDS_FN uint32_t acm_stripe_bound(uint32_t file_len, uint32_t s, uint32_t S)
{
	const uint32_t slot = ((file_len + 15u) & ~15u) + 16u;
	return s >= S ? slot : (uint32_t)(((uint64_t)slot * s / S) & ~15ull);
}

/* first block of block range r of R of a stream of `blocks` blocks (r == R: its end).  Ranges are cut at multiples of `unit` blocks (0 / 1:
 * anywhere; acm_batch.cpp asks for whole tiles of the lean kernel where a stream has the byte-plane form, which also keeps every row pair
 * of an odd block height inside one range); a short stream may have empty ranges */
ACM_BOUNDS_FN uint32_t acm_range_bound(uint32_t blocks, uint32_t r, uint32_t R, uint32_t unit)
{
	if (r >= R)
		return blocks;
	const uint32_t b = (uint32_t)((uint64_t)blocks * r / R);
	return unit > 1u ? b / unit * unit : b;
}

#endif
