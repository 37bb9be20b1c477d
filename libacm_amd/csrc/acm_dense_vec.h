/*
 * acm_dense_vec.h - what every dense kernel shares (acm_dense_gather.h's gather and acm_dense_overlay.hip stand on it): the cut of a
 * sub-row into the samples in front of its first aligned output line, whole vectors and the samples behind them, the aligned 16-byte
 * line loads funnelled by a wavefront-uniform shift, and the whole-line stores of int16 and float32 vectors.  Device code, in an
 * unnamed namespace of the including file.  The units and the grid are acm_dense_geo.h's.
 */
#ifndef ACM_DENSE_VEC_H
#define ACM_DENSE_VEC_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "acm_dense_geo.h"

namespace {

using namespace acm_dense;

constexpr uint32_t DENSE_MAX_GRID = ACM_CAP_DENSE_GRID;    /* workgroups of a launch at most (dense_geo's `most`); the kernels stride over the rest */

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

/* A sub-row of sub_len output samples at o: [0, head) in front of the first aligned 16-byte output line, nvec whole vectors - the
 * body, whose lanes store whole lines (one of int16, two of float32) -, [tail, sub_len) behind them.  Lane t of unit u has vector
 * u * DENSE_BLOCK + t; the up to 7 samples in front are unit 0's and the up to 7 behind the last unit's, with narrow accesses */
struct SubCut {
	uint64_t head, nvec, tail;
};
template <typename OUT> __device__ __forceinline__ SubCut cut_sub_row(const OUT *o, uint64_t sub_len)
{
	const uint64_t to_line = ((0u - (uint32_t)reinterpret_cast<uintptr_t>(o)) & 15u) / sizeof(OUT);
	SubCut c;
	c.head = to_line < sub_len ? to_line : sub_len;
	c.nvec = (sub_len - c.head) / DENSE_VEC;
	c.tail = c.head + c.nvec * DENSE_VEC;
	return c;
}

/* how far into its aligned 16-byte line the source of the body's first vector lies: the same for every vector of the sub-row, since
 * consecutive vectors' sources are a whole number of lines apart */
__device__ __forceinline__ uint32_t line_shift(const int16_t *first)
{
	return (uint32_t)reinterpret_cast<uintptr_t>(first) & 15u;
}

template <bool NT, typename V> __device__ __forceinline__ void store_line(V *at, V v)
{
	if (NT)
		__builtin_nontemporal_store(v, at);
	else
		*at = v;
}

/* the NDW dwords from p on: p lies sh (even, wavefront-uniform) bytes into an aligned 16-byte line, and bytes [sh, sh + used) counted
 * from that line are samples the caller may read; e[j] is dword j, whole up to byte `used`.  LINES aligned lines can hold a part of them */
template <int NDW, int LINES> __device__ __forceinline__ void load_dwords(const int16_t *p, uint32_t sh, uint32_t used, uint32_t (&e)[NDW])
{
	static_assert(4 * LINES > NDW, "the funnel reads dword NDW");
	const u32x4 *line = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(p) - sh);
	uint32_t d[4 * LINES];
#pragma unroll
	for (int v = 0; v < LINES; v++) {
		u32x4 x = { 0, 0, 0, 0 };
		if (16u * v < sh + used)                                /* a line behind the vector's last sample is not touched */
			x = line[v];
		d[4 * v] = x.x;
		d[4 * v + 1] = x.y;
		d[4 * v + 2] = x.z;
		d[4 * v + 3] = x.w;
	}
	/* whole dwords of the shift: d[i] <- d[i + (sh >> 2)], for the NDW + 1 dwords the funnel reads */
	if (sh & 4) {
#pragma unroll
		for (int i = 0; i + 1 < 4 * LINES; i++)
			d[i] = d[i + 1];
	}
	if (sh & 8) {
#pragma unroll
		for (int i = 0; i + 2 < 4 * LINES; i++)
			d[i] = d[i + 2];
	}
	const uint32_t r = sh & 3;                                      /* 0 or 2 */
#pragma unroll
	for (int j = 0; j < NDW; j++)
		e[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], r);
}

/* 8 samples from p on, every STRIDE-th: p lies sh (even, wavefront-uniform) bytes into an aligned 16-byte line */
template <int STRIDE> __device__ __forceinline__ void load_vec(const int16_t *p, uint32_t sh, int (&s)[DENSE_VEC])
{
	/* STRIDE + 1 aligned lines can hold a part of the vector's bytes, [sh, sh + 16) or [sh, sh + 30) counted from the first line */
	uint32_t e[4 * STRIDE];
	load_dwords<4 * STRIDE, STRIDE + 1>(p, sh, STRIDE == 1 ? 16 : 30, e);
#pragma unroll
	for (int j = 0; j < 4 * STRIDE; j++) {
		if (STRIDE == 1) {
			s[2 * j] = (int16_t)(e[j] & 0xFFFFu);
			s[2 * j + 1] = (int16_t)(e[j] >> 16);
		} else {
			s[j] = (int16_t)(e[j] & 0xFFFFu);               /* the other channel's sample is the high half */
		}
	}
}

template <bool NT> __device__ __forceinline__ void store_vec(int16_t *at, const int (&s)[DENSE_VEC])
{
	u32x4 w;
	w.x = ((uint32_t)s[0] & 0xFFFFu) | ((uint32_t)s[1] << 16);
	w.y = ((uint32_t)s[2] & 0xFFFFu) | ((uint32_t)s[3] << 16);
	w.z = ((uint32_t)s[4] & 0xFFFFu) | ((uint32_t)s[5] << 16);
	w.w = ((uint32_t)s[6] & 0xFFFFu) | ((uint32_t)s[7] << 16);
	store_line<NT>(reinterpret_cast<u32x4 *>(at), w);
}

__device__ __forceinline__ float to_out(float *, int s) { return (float)s * 0x1p-15f; }
__device__ __forceinline__ int16_t to_out(int16_t *, int s) { return (int16_t)s; }

template <bool NT> __device__ __forceinline__ void store_vec(float *at, const int (&s)[DENSE_VEC])
{
	f32x4 a, b;
	a.x = to_out(at, s[0]);
	a.y = to_out(at, s[1]);
	a.z = to_out(at, s[2]);
	a.w = to_out(at, s[3]);
	b.x = to_out(at, s[4]);
	b.y = to_out(at, s[5]);
	b.z = to_out(at, s[6]);
	b.w = to_out(at, s[7]);
	store_line<NT>(reinterpret_cast<f32x4 *>(at), a);
	store_line<NT>(reinterpret_cast<f32x4 *>(at) + 1, b);
}

} // namespace

#endif
