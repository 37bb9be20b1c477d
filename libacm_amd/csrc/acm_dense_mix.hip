/*
 * acm_dense_mix.hip - acm_dense.hip's gather for a call with ACM_DENSE_MIX (include/acm_hip.h) in which some window's file has the
 * other channel count than the batch: the rows of such windows are converted on the way, the others are laid out as acm_dense_rows
 * lays them out.  Launched only where the row table says that a row converts (acm_dense_layout.cpp); every other call keeps
 * acm_dense_rows, untouched.
 *
 * No counterpart in the reference.  A row's record carries its mode in the high bits of `count` (acm_device.h); a build of the kernel
 * is one layout of the batch, and a layout has one converting mode beside the plain one:
 *
 *   layout                    plain row (mode bits 0)            converting row
 *   MONO     C = 1            copy                               DOWN       out[i] = (L_i + R_i) >> 1: 32-bit sum, arithmetic shift
 *   INTER    C = 2 [T][2]     copy                               UP_INTER   out[2i] = out[2i + 1] = s_i
 *   PLANAR   C = 2 [2][T]     split into a plane per channel     UP_PLANAR  out[i] = out[T + i] = s_i: both planes copy the row
 *
 * float32 is the int16 result times 2^-15, so the down-mix has one definition, made on integers.
 *
 * The geometry is acm_dense_rows': sub-rows (one, or one per plane), units of 256 lanes, a flat grid that strides over (row, sub-row,
 * unit).  A workgroup works on one row, so the mode is a wavefront-uniform branch between two instances of one body.  That body
 * starts where the OUTPUT is 16-byte aligned; a lane stores whole 16-byte lines and loads the aligned 16-byte lines that hold its
 * source bytes, funnelled by a shift that is the same for every vector of the sub-row (acm_dense_vec.h).  A line is loaded only if it
 * holds a sample the vector needs, so every load lies inside the row's own samples rounded out to 16 bytes, which a window's
 * 64-sample slot contains.  What a vector of 8 outputs needs, counted from its first source byte:
 *
 *   copy, UP_PLANAR   16 bytes    two lines at most
 *   split             30 bytes    three lines at most (the last sample's neighbour is not the row's)
 *   DOWN              32 bytes    three lines at most: both samples of the last frame
 *   UP_INTER          see below
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
 * samples end.  No LDS, no scratch (every register array is indexed by constants after unrolling).  Temporal stores: the batch is
 * read by the next kernel of the caller's step (profiles/dense_crop_notes.txt).
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "acm_dense_vec.h"
#include "acm_device.h"

namespace {

enum Layout { MONO = 0, INTER = 1, PLANAR = 2 };
enum Path { COPY, SPLIT, DOWN, UP_INTER };      /* what a sub-row does with its source; UP_PLANAR is COPY in both planes */

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

/* one unit of one sub-row: `have` output samples from `sub`, zeros behind them up to sub_len */
template <typename OUT, Path P>
__device__ __forceinline__ void sub_row(const int16_t *sub, uint64_t have, OUT *o, uint64_t sub_len, uint32_t unit, uint32_t units)
{
	constexpr int PER_LANE = P == UP_INTER ? 2 : 1;         /* vectors of 8 outputs a body lane writes */
	/* [0, head) in front of the first aligned output line, nvec whole vectors, [tail, sub_len) behind them */
	const uint64_t to_line = ((0u - (uint32_t)reinterpret_cast<uintptr_t>(o)) & 15u) / sizeof(OUT);
	const uint64_t head = to_line < sub_len ? to_line : sub_len;
	const uint64_t nvec = (sub_len - head) / DENSE_VEC;
	const uint64_t tail = head + nvec * DENSE_VEC;
	/* the source of the body's first vector, and how far into its aligned line it lies */
	const int16_t *first = P == COPY ? sub + head : P == UP_INTER ? sub + head / 2 : sub + 2 * head;
	const uint32_t sh = (uint32_t)reinterpret_cast<uintptr_t>(first) & 15u;
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
		store_vec<false>(o + e, s[0]);
		if (two)
			store_vec<false>(o + e + DENSE_VEC, s[PER_LANE - 1]);
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

/* sub_len: output samples of a sub-row (frames with PLANAR, else the whole row); units: workgroups per sub-row */
template <typename OUT, int LAYOUT>
__global__ __launch_bounds__(DENSE_BLOCK) void acm_dense_mixed(const int16_t *__restrict__ src, const AcmDenseRow *__restrict__ rows, uint64_t nwork,
								uint32_t units, OUT *__restrict__ out, uint64_t row_len, uint64_t sub_len)
{
	constexpr uint32_t SUBS = LAYOUT == PLANAR ? 2 : 1;
	const uint32_t per_row = units * SUBS;
	for (uint64_t work = blockIdx.x; work < nwork; work += gridDim.x) {
		const uint64_t k = work / per_row;
		const uint32_t rem = (uint32_t)(work - k * per_row);
		const uint32_t plane = SUBS == 2 ? rem / units : 0;
		const uint32_t unit = rem - plane * units;
		const AcmDenseRow row = rows[k];
		const bool converts = (row.count >> ACM_DENSE_MODE_SHIFT) != 0;
		const uint64_t count = row.count & ACM_DENSE_COUNT_MASK;
		const int16_t *from = src + row.src;
		OUT *o = out + k * row_len + (uint64_t)plane * sub_len;
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
			else            /* every second sample of row.count, from sample `plane` on */
				sub_row<OUT, SPLIT>(from + plane, (count + 1 - plane) / 2, o, sub_len, unit, units);
		}
	}
}

template <typename OUT, int LAYOUT>
int launch(uint32_t grid, hipStream_t st, const int16_t *d_src, const AcmDenseRow *d_rows, uint64_t nwork, uint32_t units, void *d_out, uint64_t row_len,
	   uint64_t sub_len)
{
	hipLaunchKernelGGL((acm_dense_mixed<OUT, LAYOUT>), dim3(grid), dim3(DENSE_BLOCK), 0, st, d_src, d_rows, nwork, units, static_cast<OUT *>(d_out),
			   row_len, sub_len);
	return (int)hipGetLastError();
}

} // namespace

extern "C" int acmk_launch_dense_mixed(const int16_t *d_src, const AcmDenseRow *d_rows, uint64_t nrows, void *d_out, uint64_t frames, uint32_t channels,
				       int planar, int f32, uint32_t dense_grid, void *stream)
{
	if (nrows == 0)
		return 0;
	const int layout = channels == 1 ? MONO : planar ? PLANAR : INTER;
	const int subs = layout == PLANAR ? 2 : 1;
	const uint64_t row_len = frames * channels, sub_len = subs == 2 ? frames : row_len;
	const uint64_t units = std::max<uint64_t>(1, (sub_len / DENSE_VEC + DENSE_BLOCK - 1) / DENSE_BLOCK);
	if (units > 0x7FFFFFFFull || nrows > ~0ull / (units * subs))
		return (int)hipErrorInvalidValue;
	const uint64_t nwork = nrows * units * subs;
	const uint32_t grid = (uint32_t)std::min<uint64_t>(nwork, acm_cap_value(dense_grid, DENSE_MAX_GRID));
	hipStream_t st = (hipStream_t)stream;
#define ACM_MIX_LAUNCH(OUT, LAYOUT) launch<OUT, LAYOUT>(grid, st, d_src, d_rows, nwork, (uint32_t)units, d_out, row_len, sub_len)
	if (f32)
		return layout == MONO ? ACM_MIX_LAUNCH(float, MONO) : layout == INTER ? ACM_MIX_LAUNCH(float, INTER) : ACM_MIX_LAUNCH(float, PLANAR);
	return layout == MONO ? ACM_MIX_LAUNCH(int16_t, MONO) : layout == INTER ? ACM_MIX_LAUNCH(int16_t, INTER) : ACM_MIX_LAUNCH(int16_t, PLANAR);
#undef ACM_MIX_LAUNCH
}
