/*
 * acm_dense_mix.hip - acm_dense.hip's gather for a call with ACM_DENSE_MIX (include/acm_hip.h) in which some window's file has the
 * other channel count than the batch: the rows of such windows are converted on the way, the others are laid out as acm_dense_rows
 * lays them out.  Launched only where the row table says that a row converts (acm_dense_layout.cpp); every other call keeps
 * acm_dense_rows, untouched.
 *
 * No counterpart in the reference.  A row's record carries its mode in the high bits of `count` (acm_device.h); a build of the kernel
 * is one layout of the batch, and a layout has one converting mode beside the plain one - DOWN for MONO, UP_INTER for INTER,
 * UP_PLANAR for PLANAR (the table at plain_sub_row, acm_dense_gather.h).  A workgroup works on one row, so the mode is a
 * wavefront-uniform branch between two instances of one body.  The geometry, the funnel, what each path loads and the body itself are
 * that header's.  No LDS, no scratch.  Temporal stores: the batch is read by the next kernel of the caller's step
 * (profiles/dense_crop_notes.txt).
 */
#include <hip/hip_runtime.h>

#include "acm_dense_gather.h"

namespace {

/* sub_len: output samples of a sub-row (frames with PLANAR, else the whole row); units: workgroups per sub-row */
template <typename OUT, int LAYOUT>
__global__ __launch_bounds__(DENSE_BLOCK) void acm_dense_mixed(const int16_t *__restrict__ src, const AcmDenseRow *__restrict__ rows, uint64_t nwork,
								uint32_t units, OUT *__restrict__ out, uint64_t row_len, uint64_t sub_len)
{
	for (uint64_t work = blockIdx.x; work < nwork; work += gridDim.x) {
		const WorkItem w = work_item<LAYOUT == PLANAR ? 2 : 1>(work, units);
		const AcmDenseRow row = rows[w.row];
		const bool converts = (row.count >> ACM_DENSE_MODE_SHIFT) != 0;
		OUT *o = out + w.row * row_len + (uint64_t)w.plane * sub_len;
		plain_sub_row<OUT, LAYOUT>(src + row.src, converts, row.count & ACM_DENSE_COUNT_MASK, w.plane, o, sub_len, w.unit, units);
	}
}

} // namespace

extern "C" int acmk_launch_dense_mixed(const int16_t *d_src, const AcmDenseRow *d_rows, uint64_t nrows, void *d_out, uint64_t frames, uint32_t channels,
				       int planar, int f32, uint32_t dense_grid, void *stream)
{
	if (nrows == 0)
		return 0;
	const DenseGeo g = dense_geo(nrows, frames, channels, planar, dense_grid, DENSE_MAX_GRID);
	if (!g.ok)
		return (int)hipErrorInvalidValue;
	return dense_dispatch(f32, g.layout, [&](auto o, auto layout) {
		using OUT = decltype(o);
		hipLaunchKernelGGL((acm_dense_mixed<OUT, decltype(layout)::value>), dim3(g.grid), dim3(DENSE_BLOCK), 0, (hipStream_t)stream, d_src, d_rows,
				   g.nwork, g.units, static_cast<OUT *>(d_out), g.row_len, g.sub_len);
		return (int)hipGetLastError();
	});
}
