/*
 * acm_dense_overlay.hip - the launches acm_batch_decode_windows_overlay (acm_batch_windows.cpp) puts behind a dense call's gather
 * launch: the energies of the source rows, a gain per output row, and the output rows combined from them (include/acm_hip.h: volume,
 * and a second crop laid over the first at a signal-to-noise ratio).
 *
 * No counterpart in the reference.  The source rows lie in an arena of the handle's own, row k at sample k * R - any 2-byte alignment
 * - as int16, written by the gather launch in front of these on the same stream.  The two large kernels stand on the dense kernels'
 * unit (acm_dense_geo.h: 256 lanes, 8 samples a lane, 2048 samples a unit) and on acm_dense_vec.h's aligned 16-byte line loads,
 * funnelled by a shift that is the same for every vector of a row.
 *
 * acm_dense_energy: a flat grid over (marked source row, unit).  A lane squares its 8 samples (the last vector of a row sample by
 * sample) into a 64-bit sum, a wavefront adds its lanes by shuffles, the workgroup its four wavefronts through 32 bytes of LDS, and
 * one 64-bit integer atomic add per workgroup goes to the row's energy.  Integer sums do not depend on the order of arrival: the
 * energies, and everything made from them, are the same in every run.
 *
 * acm_dense_overlay: a flat grid over (output row, unit).  As in every gather (cut_sub_row, acm_dense_vec.h) the body of a row starts
 * where the OUTPUT is 16-byte aligned and stores whole lines (one of int16, two of float32), with single elements in front and
 * behind; A and B have a shift each.  A row without b loads no B - the branch is the workgroup's.  No LDS, no scratch.
 *
 * acm_dense_gains, between the two: a lane per output row derives the row's g from the two energies (16 products of 128 bits,
 * acm_overlay_layout.h - the text acm_dense_overlay_gain compiles too) and stores the row's result, once; the combine kernel reads g
 * from there.  (Derived by every workgroup of the combine kernel for itself, those products were half of that kernel's time:
 * profiles/dense_overlay_notes.txt.)
 */
#include <hip/hip_runtime.h>

#include "acm_dense_vec.h"
#include "acm_device.h"
#include "acm_overlay_layout.h"

namespace {

constexpr int WAVE = 64;

__global__ __launch_bounds__(DENSE_BLOCK) void acm_dense_energy(const int16_t *__restrict__ src, const uint32_t *__restrict__ marked, uint64_t nwork,
								 uint32_t units, uint64_t row_len, unsigned long long *__restrict__ energy)
{
	__shared__ unsigned long long part[DENSE_BLOCK / WAVE];
	for (uint64_t work = blockIdx.x; work < nwork; work += gridDim.x) {
		const uint64_t i = work / units;
		const uint32_t unit = (uint32_t)(work - i * units);
		const uint32_t k = marked[i];
		const int16_t *row = src + (uint64_t)k * row_len;
		const uint32_t sh = (uint32_t)reinterpret_cast<uintptr_t>(row) & 15u;
		const uint64_t e = (uint64_t)unit * DENSE_UNIT +threadIdx.x * DENSE_VEC;
		unsigned long long sum = 0;
		if (e + DENSE_VEC <= row_len) {
			int s[DENSE_VEC];
			load_vec<1>(row + e, sh, s);
#pragma unroll
			for (int j = 0; j < DENSE_VEC; j++)
				sum += (uint32_t)(s[j] * s[j]);
		} else {
#pragma unroll
			for (int j = 0; j < DENSE_VEC; j++) {
				const int x = e + j < row_len ? row[e + j] : 0;
				sum += (uint32_t)(x * x);
			}
		}
#pragma unroll
		for (int off = WAVE / 2; off; off >>= 1)
			sum += __shfl_xor(sum, off, WAVE);
		if ((threadIdx.x & (WAVE - 1)) == 0)
			part[threadIdx.x / WAVE] = sum;
		__syncthreads();
		if (threadIdx.x == 0) {
			unsigned long long all = 0;
#pragma unroll
			for (int w = 0; w < DENSE_BLOCK / WAVE; w++)
				all += part[w];
			atomicAdd(&energy[k], all);
		}
		__syncthreads();                /* the next piece of work writes part[] again */
	}
}

__global__ __launch_bounds__(DENSE_BLOCK) void acm_dense_gains(const AcmOverlayRow *__restrict__ rows, const unsigned long long *__restrict__ energy,
								AcmOverlayResult *__restrict__ res, uint64_t nrows)
{
	const uint64_t r = (uint64_t)blockIdx.x * DENSE_BLOCK + threadIdx.x;
	if (r >= nrows)
		return;
	const AcmOverlayRow row = rows[r];
	unsigned long long ea = 0, eb = 0;
	uint32_t g = 0;
	if (row.b != ACM_OVERLAY_NONE && row.snr) {
		ea = energy[row.a];
		eb = energy[row.b];
		g = acm_overlay_gain(ea, eb, row.snr);
	} else if (row.b != ACM_OVERLAY_NONE) {
		g = row.gain;
	}
	res[r] = AcmOverlayResult{ g, ea, eb };
}

/* y of include/acm_hip.h from one sample of A and one of B.  |m * vol + 2^23| < 2^48, so the shifted value is an int and clamps as one */
__device__ __forceinline__ int combine(int a, int b, int g, int vol)
{
	const int m = 4096 * a + g * b;
	const int y = (int)(((long long)m * vol + (1ll << 23)) >> 24);
	return y < -32768 ? -32768 : y > 32767 ? 32767 : y;
}

template <typename OUT>
__global__ __launch_bounds__(DENSE_BLOCK) void acm_dense_overlay(const int16_t *__restrict__ src, const AcmOverlayRow *__restrict__ rows,
								  const AcmOverlayResult *__restrict__ res, uint64_t nwork, uint32_t units, OUT *__restrict__ out,
								  uint64_t row_len)
{
	for (uint64_t work = blockIdx.x; work < nwork; work += gridDim.x) {
		const uint64_t r = work / units;
		const uint32_t unit = (uint32_t)(work - r * units);
		const AcmOverlayRow row = rows[r];
		const bool over = row.b != ACM_OVERLAY_NONE;
		const int gi = (int)res[r].gain, vol = (int)row.vol;
		const int16_t *A = src + (uint64_t)row.a * row_len;
		const int16_t *B = src + (uint64_t)(over ? row.b : row.a) * row_len;
		OUT *o = out + r * row_len;
		const SubCut c = cut_sub_row(o, row_len);
		const uint64_t head = c.head, nvec = c.nvec, tail = c.tail;
		const uint32_t sha = line_shift(A + head), shb = line_shift(B + head);

		const uint64_t v = (uint64_t)unit * DENSE_BLOCK + threadIdx.x;
		if (v < nvec) {
			const uint64_t e = head + v * DENSE_VEC;
			int s[DENSE_VEC], t[DENSE_VEC];
			load_vec<1>(A + e, sha, s);
			if (over) {
				load_vec<1>(B + e, shb, t);
#pragma unroll
				for (int j = 0; j < DENSE_VEC; j++)
					s[j] = combine(s[j], t[j], gi, vol);
			} else {
#pragma unroll
				for (int j = 0; j < DENSE_VEC; j++)
					s[j] = combine(s[j], 0, 0, vol);
			}
			store_vec<false>(o + e, s);
		}
		if (unit == 0 && threadIdx.x < head) {
			const uint64_t e = threadIdx.x;
			o[e] = to_out(o, combine(A[e], over ? B[e] : 0, gi, vol));
		}
		if (unit == units - 1 && tail + threadIdx.x < row_len) {
			const uint64_t e = tail + threadIdx.x;
			o[e] = to_out(o, combine(A[e], over ? B[e] : 0, gi, vol));
		}
	}
}

} // namespace

extern "C" int acmk_launch_dense_energy(const int16_t *d_src, const uint32_t *d_marked, uint64_t nmarked, uint64_t row_len, uint64_t *d_energy,
					uint32_t dense_grid, void *stream)
{
	if (nmarked == 0 || row_len == 0)
		return 0;
	/* rows of one sub-row; every sample is in a vector here, so the units are whole */
	const DenseGeo g = dense_geo(nmarked, row_len, 1, 0, dense_grid, DENSE_MAX_GRID, true);
	if (!g.ok)
		return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL(acm_dense_energy, dim3(g.grid), dim3(DENSE_BLOCK), 0, (hipStream_t)stream, d_src, d_marked, g.nwork, g.units, row_len,
			   reinterpret_cast<unsigned long long *>(d_energy));
	return (int)hipGetLastError();
}

extern "C" int acmk_launch_dense_overlay(const int16_t *d_src, const AcmOverlayRow *d_rows, const uint64_t *d_energy, AcmOverlayResult *d_res,
					 uint64_t nrows, void *d_out, uint64_t row_len, int f32, uint32_t dense_grid, void *stream)
{
	if (nrows == 0 || row_len == 0)
		return 0;
	const DenseGeo g = dense_geo(nrows, row_len, 1, 0, dense_grid, DENSE_MAX_GRID);
	if (!g.ok)
		return (int)hipErrorInvalidValue;
	const unsigned long long *energy = reinterpret_cast<const unsigned long long *>(d_energy);
	hipStream_t st = (hipStream_t)stream;
	const uint64_t gain_grid = (nrows + DENSE_BLOCK - 1) / DENSE_BLOCK;
	if (gain_grid > 0x7FFFFFFFull)
		return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL(acm_dense_gains, dim3((uint32_t)gain_grid), dim3(DENSE_BLOCK), 0, st, d_rows, energy, d_res, nrows);
	const int e = (int)hipGetLastError();
	if (e != 0)
		return e;
	if (f32)
		hipLaunchKernelGGL(acm_dense_overlay<float>, dim3(g.grid), dim3(DENSE_BLOCK), 0, st, d_src, d_rows, d_res, g.nwork, g.units,
				   static_cast<float *>(d_out), row_len);
	else
		hipLaunchKernelGGL(acm_dense_overlay<int16_t>, dim3(g.grid), dim3(DENSE_BLOCK), 0, st, d_src, d_rows, d_res, g.nwork, g.units,
				   static_cast<int16_t *>(d_out), row_len);
	return (int)hipGetLastError();
}
