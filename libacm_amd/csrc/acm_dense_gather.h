/*
 * acm_dense_gather.h - the gather of a dense crop batch, written once for its four kernels (acm_dense.hip, acm_dense_mix.hip,
 * acm_dense_resample.hip, acm_dense_speed.hip): which (row, sub-row, unit) a piece of work is, and one unit of one sub-row of a
 * row that is not filtered - copied, split into planes, down- or up-mixed.  Device code, in an unnamed namespace of the including
 * file.
 *
 * The geometry (acm_dense_geo.h): a row is cut into sub-rows (one, or one per plane) and a sub-row into units of 256 lanes and 8
 * output samples a lane, a workgroup each; the grid is flat over (row, sub-row, unit) and strides.  A workgroup works on one row,
 * so what the row does - its mode, whether it is filtered - is a wavefront-uniform branch.
 *
 * The funnel (acm_dense_vec.h): the body of a sub-row starts where the OUTPUT is 16-byte aligned, so every lane stores whole
 * 16-byte lines (one of int16, two of float32).  The source of such a vector sits `sh` bytes into an aligned 16-byte line, the same
 * sh for every vector of the sub-row: the lane loads the aligned lines that hold its source bytes and funnels them - whole dwords
 * by selects, the odd half dword by v_alignbyte.  A line is loaded only if it holds a sample the vector needs, so every load lies
 * inside the row's own samples rounded out to 16 bytes, which a window's 64-sample slot contains.  What a vector of 8 outputs
 * needs, counted from its first source byte:
 *
 *   COPY (and UP_PLANAR: both planes copy the row)   16 bytes    two lines at most
 *   SPLIT                                            30 bytes    three lines at most (the last sample's neighbour is not the row's)
 *   DOWN                                             32 bytes    three lines at most: both samples of the last frame
 *   UP_INTER                                         see below
 *
 * UP_INTER has two outputs per source sample, so consecutive vectors of 8 outputs are 8 source bytes apart and their shifts would
 * alternate.  Chosen here: a lane produces 16 outputs - two lines of int16, four of float32 - from ONE load of 8 source samples (9
 * where the body starts on the second copy of a sample: a tensor that begins an odd number of elements from a 16-byte line, int16 or
 * float32, makes it do so), so the lanes' source vectors are 16 bytes apart and the shift stays uniform.  The units are still cut
 * for 8 outputs a lane: of an UP_INTER row's units the second half has no vector and only the last one writes the tail.  Where the
 * body has an odd number of 8-output vectors the last lane loads and stores for its first line only, so the tail stays below 8
 * samples.
 *
 * Narrow accesses: the up to 7 samples in front of the body, the up to 7 behind it, and the one vector in which a short row's
 * samples end.  No LDS, no scratch (every register array is indexed by constants after unrolling).
 */
#ifndef ACM_DENSE_GATHER_H
#define ACM_DENSE_GATHER_H

#include <type_traits>

#include "acm_dense_vec.h"
#include "acm_device.h"

namespace {

enum Path { COPY, SPLIT, DOWN, UP_INTER };      /* what a sub-row does with its source; UP_PLANAR is COPY in both planes */

/* piece `work` of a launch with SUBS sub-rows a row and `units` units a sub-row: the sub-row begins at element
 * row * row_len + plane * sub_len of the output */
struct WorkItem {
	uint64_t row;
	uint32_t plane, unit;
};
template <uint32_t SUBS> __device__ __forceinline__ WorkItem work_item(uint64_t work, uint32_t units)
{
	const uint32_t per_row = units * SUBS;
	WorkItem w;
	w.row = work / per_row;
	const uint32_t rem = (uint32_t)(work - w.row * per_row);
	w.plane = SUBS == 2 ? rem / units : 0;
	w.unit = rem - w.plane * units;
	return w;
}

/* output sample e of a sub-row whose source starts at sub, e below what the sub-row has */
template <Path P> __device__ __forceinline__ int sample(const int16_t *sub, uint64_t e)
{
	if (P == COPY)
		return sub[e];
	if (P == SPLIT)
		return sub[2 * e];
	if (P == DOWN)
		return ((int)sub[2 * e] + (int)sub[2 * e + 1]) >> 1;
	return sub[e >> 1];
}

/* one unit of one sub-row: `have` output samples from `sub`, zeros behind them up to sub_len.  NT: non-temporal line stores */
template <typename OUT, Path P, bool NT = false>
__device__ __forceinline__ void sub_row(const int16_t *sub, uint64_t have, OUT *o, uint64_t sub_len, uint32_t unit, uint32_t units)
{
	constexpr int PER_LANE = P == UP_INTER ? 2 : 1;         /* vectors of 8 outputs a body lane writes */
	const SubCut c = cut_sub_row(o, sub_len);
	const uint64_t head = c.head, nvec = c.nvec, tail = c.tail;
	/* the source of the body's first vector, and how far into its aligned line it lies */
	const uint32_t sh = line_shift(P == COPY ? sub + head : P == UP_INTER ? sub + head / 2 : sub + 2 * head);
	const uint32_t odd = P == UP_INTER ? (uint32_t)head & 1u : 0;  /* the body starts on the second copy of a sample */

	const uint64_t v = ((uint64_t)unit * DENSE_BLOCK + threadIdx.x) * PER_LANE;
	if (v < nvec) {
		const uint64_t e = head + v * DENSE_VEC;
		const bool two = PER_LANE == 2 && v + 1 < nvec;
		const uint32_t outs = two ? 2 * DENSE_VEC : DENSE_VEC;  /* outputs this lane stores */
		int s[PER_LANE][DENSE_VEC];
		if (e + outs <= have) {
			if (P == COPY) {
				load_vec<1>(sub + e, sh, s[0]);
			} else if (P == SPLIT) {
				load_vec<2>(sub + 2 * e, sh, s[0]);
			} else if (P == DOWN) {
				uint32_t d[DENSE_VEC];
				load_dwords<DENSE_VEC, 3>(sub + 2 * e, sh, 32, d);
#pragma unroll
				for (int i = 0; i < DENSE_VEC; i++)
					s[0][i] = ((int)(int16_t)(d[i] & 0xFFFFu) + (int)(int16_t)(d[i] >> 16)) >> 1;
			} else {
				/* samples t[0 .. outs / 2 + odd) from sample e / 2 on; output e + i is t[(i + odd) / 2] */
				uint32_t d[5];
				load_dwords<5, 2>(sub + e / 2, sh, outs + 2 * odd, d);
				int t[10];
#pragma unroll
				for (int j = 0; j < 5; j++) {
					t[2 * j] = (int16_t)(d[j] & 0xFFFFu);
					t[2 * j + 1] = (int16_t)(d[j] >> 16);
				}
#pragma unroll
				for (int i = 0; i < PER_LANE * DENSE_VEC; i++)
					s[i / DENSE_VEC][i % DENSE_VEC] = odd ? t[(i + 1) / 2] : t[i / 2];
			}
		} else {
#pragma unroll
			for (int i = 0; i < PER_LANE * DENSE_VEC; i++)
				s[i / DENSE_VEC][i % DENSE_VEC] = i < outs && e + i < have ? sample<P>(sub, e + i) : 0;
		}
		store_vec<NT>(o + e, s[0]);
		if (two)
			store_vec<NT>(o + e + DENSE_VEC, s[PER_LANE - 1]);
	}
	if (unit == 0 && threadIdx.x < head) {
		const uint64_t e = threadIdx.x;
		o[e] = to_out(o, e < have ? sample<P>(sub, e) : 0);
	}
	if (unit == units - 1 && tail + threadIdx.x < sub_len) {
		const uint64_t e = tail + threadIdx.x;
		o[e] = to_out(o, e < have ? sample<P>(sub, e) : 0);
	}
}

/* ... of a row of a batch of one LAYOUT.  from, count: the row's source samples; converts: its record carries a mode (acm_device.h:
 * AcmDenseMode) - a layout has one converting mode beside the plain one.  float32 is the int16 result times 2^-15, so the down-mix
 * has one definition, made on integers
 *
 *   layout                    plain row (mode bits 0)            converting row
 *   MONO     C = 1            copy                               DOWN       out[i] = (L_i + R_i) >> 1: 32-bit sum, arithmetic shift
 *   INTER    C = 2 [T][2]     copy                               UP_INTER   out[2i] = out[2i + 1] = s_i
 *   PLANAR   C = 2 [2][T]     split into a plane per channel     UP_PLANAR  out[i] = out[T + i] = s_i: both planes copy the row
 */
template <typename OUT, int LAYOUT>
__device__ __forceinline__ void plain_sub_row(const int16_t *from, bool converts, uint64_t count, uint32_t plane, OUT *o, uint64_t sub_len,
					      uint32_t unit, uint32_t units)
{
	if (LAYOUT == MONO) {
		if (converts)
			sub_row<OUT, DOWN>(from, count / 2, o, sub_len, unit, units);
		else
			sub_row<OUT, COPY>(from, count, o, sub_len, unit, units);
	} else if (LAYOUT == INTER) {
		if (converts)
			sub_row<OUT, UP_INTER>(from, 2 * count, o, sub_len, unit, units);
		else
			sub_row<OUT, COPY>(from, count, o, sub_len, unit, units);
	} else {
		if (converts)
			sub_row<OUT, COPY>(from, count, o, sub_len, unit, units);
		else            /* every second sample of the row, from sample `plane` on */
			sub_row<OUT, SPLIT>(from + plane, (count + 1 - plane) / 2, o, sub_len, unit, units);
	}
}

/* the build of a kernel template <typename OUT, int LAYOUT> a launch takes: launch(OUT(), std::integral_constant<int, LAYOUT>()) */
template <typename F> int dense_dispatch(int f32, int layout, F &&launch)
{
	using M = std::integral_constant<int, MONO>;
	using I = std::integral_constant<int, INTER>;
	using P = std::integral_constant<int, PLANAR>;
	if (f32)
		return layout == MONO ? launch(float(), M()) : layout == INTER ? launch(float(), I()) : launch(float(), P());
	return layout == MONO ? launch(int16_t(), M()) : layout == INTER ? launch(int16_t(), I()) : launch(int16_t(), P());
}

} // namespace

#endif
