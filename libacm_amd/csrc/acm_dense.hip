/*
 * acm_dense.hip - the last mile of a windowed decode (acm_batch_decode_windows_dense, acm_batch_windows.cpp): the crops of a call,
 * which the synthesis kernels leave at arbitrary 2-byte alignments of padded slots, laid out as equally spaced rows of one tensor.
 *
 * No counterpart in the reference.  acm_dense_rows is a pure copy: per row it reads `count` int16 samples from the PCM arena,
 * writes frames * channels output samples - the samples, then zeros - and on the way splits stereo pairs into a plane per channel
 * (STRIDE 2) and widens to float32 (the int16 sample times 2^-15, exactly what acmhip_plan_launch_f32 stores).
 *
 * The geometry, the funnel and the body of a unit are acm_dense_gather.h's, shared with acm_dense_mix.hip - the kernel that takes
 * this one's place in a call whose rows convert between mono and stereo (ACM_DENSE_MIX): this kernel is its COPY and SPLIT paths
 * alone, for a row table without mode bits.  No LDS, no scratch.
 */
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include "acm_dense_gather.h"

namespace {

/* sub_len: output samples of a sub-row (frames with STRIDE 2, else the whole row); units: workgroups per sub-row */
template <typename OUT, int STRIDE, bool NT>
__global__ __launch_bounds__(DENSE_BLOCK) void acm_dense_rows(const int16_t *__restrict__ src, const AcmDenseRow *__restrict__ rows, uint64_t nwork,
							       uint32_t units, OUT *__restrict__ out, uint64_t row_len, uint64_t sub_len)
{
	for (uint64_t work = blockIdx.x; work < nwork; work += gridDim.x) {
		const WorkItem w = work_item<STRIDE>(work, units);
		const AcmDenseRow row = rows[w.row];
		/* samples this sub-row has: every STRIDE-th of row.count, from sample `plane` on */
		const uint64_t have = STRIDE == 2 ? (row.count + 1 - w.plane) / 2 : row.count;
		OUT *o = out + w.row * row_len + (uint64_t)w.plane * sub_len;
		sub_row<OUT, STRIDE == 2 ? SPLIT : COPY, NT>(src + row.src + w.plane, have, o, sub_len, w.unit, units);
	}
}

template <typename OUT, int STRIDE> int launch(bool nt, const DenseGeo &g, hipStream_t st, const int16_t *d_src, const AcmDenseRow *d_rows, void *d_out)
{
	if (nt)
		hipLaunchKernelGGL((acm_dense_rows<OUT, STRIDE, true>), dim3(g.grid), dim3(DENSE_BLOCK), 0, st, d_src, d_rows, g.nwork, g.units,
				   static_cast<OUT *>(d_out), g.row_len, g.sub_len);
	else
		hipLaunchKernelGGL((acm_dense_rows<OUT, STRIDE, false>), dim3(g.grid), dim3(DENSE_BLOCK), 0, st, d_src, d_rows, g.nwork, g.units,
				   static_cast<OUT *>(d_out), g.row_len, g.sub_len);
	return (int)hipGetLastError();
}

} // namespace

extern "C" int acmk_launch_dense_rows(const int16_t *d_src, const AcmDenseRow *d_rows, uint64_t nrows, void *d_out, uint64_t frames, uint32_t channels,
				      int planar, int f32, uint32_t dense_grid, void *stream)
{
	if (nrows == 0)
		return 0;
	const DenseGeo g = dense_geo(nrows, frames, channels, planar, dense_grid, DENSE_MAX_GRID);
	if (!g.ok)
		return (int)hipErrorInvalidValue;
	/* Temporal stores: the batch is read by the next kernel of the caller's step (profiles/dense_crop_notes.txt).  The other variant is
	 * reachable for measurements only, like every kernel switch (acm_device.h: ACM_TUNING_ENV) */
	const char *env = ACM_TUNING_ENV("ACM_DENSE_NT");
	const bool nt = env && atoi(env) != 0;
	hipStream_t st = (hipStream_t)stream;
	if (f32)
		return g.subs == 2 ? launch<float, 2>(nt, g, st, d_src, d_rows, d_out) : launch<float, 1>(nt, g, st, d_src, d_rows, d_out);
	return g.subs == 2 ? launch<int16_t, 2>(nt, g, st, d_src, d_rows, d_out) : launch<int16_t, 1>(nt, g, st, d_src, d_rows, d_out);
}
