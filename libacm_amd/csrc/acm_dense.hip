/*
 * acm_dense.hip - the last mile of a windowed decode (acm_batch_decode_windows_dense, acm_batch_windows.cpp): the crops of a call,
 * which the synthesis kernels leave at arbitrary 2-byte alignments of padded slots, laid out as equally spaced rows of one tensor.
 *
 * No counterpart in the reference.  acm_dense_rows is a pure copy: per row it reads `count` int16 samples from the PCM arena,
 * writes frames * channels output samples - the samples, then zeros - and on the way splits stereo pairs into a plane per channel
 * (STRIDE 2) and widens to float32 (the int16 sample times 2^-15, exactly what acmhip_plan_launch_f32 stores).
 *
 * A row is cut into sub-rows (one, or one per plane) and a sub-row into units of 256 vectors of 8 output samples, a workgroup
 * each; the grid is flat over (row, plane, unit) and strides.  The body of a sub-row starts where the OUTPUT is 16-byte aligned,
 * so every lane stores whole 16-byte lines (one of int16, two of float32).  The source of such a vector sits `sh` bytes into an
 * aligned 16-byte line, the same sh for every vector of the sub-row: the lane loads the aligned lines that hold its 16 * STRIDE
 * bytes and funnels them - whole dwords by selects, the odd half dword by v_alignbyte.  A line is loaded only if it holds a
 * sample of the vector, so every load lies inside the row's own samples rounded out to 16 bytes, which a window's 64-sample
 * slot contains.  Narrow accesses: the up to 7 samples in front of the body, the up to 7 behind it, and the one vector in which a
 * short row's samples end.  No LDS, no scratch (every register array is indexed by constants after unrolling).
 *
 * The line loads, the funnel and the line stores are acm_dense_vec.h's, shared with acm_dense_mix.hip - the kernel that takes this
 * one's place in a call whose rows convert between mono and stereo (ACM_DENSE_MIX).
 */
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include <algorithm>

#include "acm_dense_vec.h"
#include "acm_device.h"

namespace {

/* sub_len: output samples of a sub-row (frames with STRIDE 2, else the whole row); units: workgroups per sub-row */
template <typename OUT, int STRIDE, bool NT>
__global__ __launch_bounds__(DENSE_BLOCK) void acm_dense_rows(const int16_t *__restrict__ src, const AcmDenseRow *__restrict__ rows, uint64_t nwork,
							       uint32_t units, OUT *__restrict__ out, uint64_t row_len, uint64_t sub_len)
{
	const uint32_t per_row = units * STRIDE;
	for (uint64_t work = blockIdx.x; work < nwork; work += gridDim.x) {
		const uint64_t k = work / per_row;
		const uint32_t rem = (uint32_t)(work - k * per_row);
		const uint32_t plane = STRIDE == 2 ? rem / units : 0;
		const uint32_t unit = rem - plane * units;
		const AcmDenseRow row = rows[k];
		/* samples this sub-row has: every STRIDE-th of row.count, from sample `plane` on */
		const uint64_t have = STRIDE == 2 ? (row.count + 1 - plane) / 2 : row.count;
		const int16_t *sub = src + row.src + plane;
		OUT *o = out + k * row_len + (uint64_t)plane * sub_len;
		/* [0, head) in front of the first aligned output line, nvec whole vectors, [tail, sub_len) behind them */
		const uint64_t to_line = ((0u - (uint32_t)reinterpret_cast<uintptr_t>(o)) & 15u) / sizeof(OUT);
		const uint64_t head = to_line < sub_len ? to_line : sub_len;
		const uint64_t nvec = (sub_len - head) / DENSE_VEC;
		const uint64_t tail = head + nvec * DENSE_VEC;
		const uint32_t sh = (uint32_t)reinterpret_cast<uintptr_t>(sub + STRIDE * head) & 15u;

		const uint64_t v = (uint64_t)unit * DENSE_BLOCK + threadIdx.x;
		if (v < nvec) {
			const uint64_t e = head + v * DENSE_VEC;
			int s[DENSE_VEC];
			if (e + DENSE_VEC <= have) {
				load_vec<STRIDE>(sub + STRIDE * e, sh, s);
			} else {
#pragma unroll
				for (int i = 0; i < DENSE_VEC; i++)
					s[i] = e + i < have ? sub[STRIDE * (e + i)] : 0;
			}
			store_vec<NT>(o + e, s);
		}
		if (unit == 0 && threadIdx.x < head) {
			const uint64_t e = threadIdx.x;
			o[e] = to_out(o, e < have ? sub[STRIDE * e] : 0);
		}
		if (unit == units - 1 && tail + threadIdx.x < sub_len) {
			const uint64_t e = tail + threadIdx.x;
			o[e] = to_out(o, e < have ? sub[STRIDE * e] : 0);
		}
	}
}

template <typename OUT, int STRIDE>
int launch(bool nt, uint32_t grid, hipStream_t st, const int16_t *d_src, const AcmDenseRow *d_rows, uint64_t nwork, uint32_t units, void *d_out,
	   uint64_t row_len, uint64_t sub_len)
{
	if (nt)
		hipLaunchKernelGGL((acm_dense_rows<OUT, STRIDE, true>), dim3(grid), dim3(DENSE_BLOCK), 0, st, d_src, d_rows, nwork, units,
				   static_cast<OUT *>(d_out), row_len, sub_len);
	else
		hipLaunchKernelGGL((acm_dense_rows<OUT, STRIDE, false>), dim3(grid), dim3(DENSE_BLOCK), 0, st, d_src, d_rows, nwork, units,
				   static_cast<OUT *>(d_out), row_len, sub_len);
	return (int)hipGetLastError();
}

} // namespace

extern "C" int acmk_launch_dense_rows(const int16_t *d_src, const AcmDenseRow *d_rows, uint64_t nrows, void *d_out, uint64_t frames, uint32_t channels,
				      int planar, int f32, uint32_t dense_grid, void *stream)
{
	if (nrows == 0)
		return 0;
	const int stride = planar && channels == 2 ? 2 : 1;
	const uint64_t row_len = frames * channels, sub_len = stride == 2 ? frames : row_len;
	const uint64_t units = std::max<uint64_t>(1, (sub_len / DENSE_VEC + DENSE_BLOCK - 1) / DENSE_BLOCK);
	if (units > 0x7FFFFFFFull || nrows > ~0ull / (units * stride))
		return (int)hipErrorInvalidValue;
	const uint64_t nwork = nrows * units * stride;
	const uint32_t grid = (uint32_t)std::min<uint64_t>(nwork, acm_cap_value(dense_grid, DENSE_MAX_GRID));
	/* Temporal stores: the batch is read by the next kernel of the caller's step (profiles/dense_crop_notes.txt).  The other variant is
	 * reachable for measurements only, like every kernel switch (acm_device.h: ACM_TUNING_ENV) */
	const char *env = ACM_TUNING_ENV("ACM_DENSE_NT");
	const bool nt = env && atoi(env) != 0;
	hipStream_t st = (hipStream_t)stream;
	if (f32)
		return stride == 2 ? launch<float, 2>(nt, grid, st, d_src, d_rows, nwork, (uint32_t)units, d_out, row_len, sub_len)
				   : launch<float, 1>(nt, grid, st, d_src, d_rows, nwork, (uint32_t)units, d_out, row_len, sub_len);
	return stride == 2 ? launch<int16_t, 2>(nt, grid, st, d_src, d_rows, nwork, (uint32_t)units, d_out, row_len, sub_len)
			   : launch<int16_t, 1>(nt, grid, st, d_src, d_rows, nwork, (uint32_t)units, d_out, row_len, sub_len);
}
