/*
 * acm_dense_resample.hip - acm_dense_mix.hip's gather for a call with ACM_DENSE_RESAMPLE (include/acm_hip.h) in which some window's
 * file has another sample rate than the batch: the rows of such windows are filtered to the batch's rate on the way, the others are
 * laid out - copied, split, down- or up-mixed - as acm_dense_mixed lays them out.  Launched only where the second row table says that
 * a row is filtered (acm_dense_layout.cpp); every other call keeps the kernel it had.
 *
 * No counterpart in the reference.  The filter, the staging of a unit and the kernel's loop are acm_dense_filter.h's, shared with
 * acm_dense_speed.hip; the geometry is every dense kernel's (acm_dense_geo.h), with 63 KB of LDS a workgroup.
 */
#include <hip/hip_runtime.h>

#include "acm_dense_filter.h"

namespace {

/* sub_len: output samples of a sub-row (frames with PLANAR, else the whole row); units: workgroups per sub-row.  A workgroup works
 * on one row, so whether the row is filtered is a workgroup-uniform branch */
template <typename OUT, int LAYOUT>
__global__ __launch_bounds__(DENSE_BLOCK) void acm_dense_resample(const int16_t *__restrict__ src, const AcmDenseRow *__restrict__ rows,
								   const AcmResampleRow *__restrict__ rs, const int16_t *__restrict__ taps, uint64_t nwork,
								   uint32_t units, OUT *__restrict__ out, uint64_t row_len, uint64_t sub_len)
{
	__shared__ __attribute__((aligned(16))) int16_t tab[TAB_CAP];
	__shared__ __attribute__((aligned(16))) int16_t xs[SPAN_CAP];
	for (uint64_t work = blockIdx.x; work < nwork; work += gridDim.x) {
		const WorkItem w = work_item<LAYOUT == PLANAR ? 2 : 1>(work, units);
		const AcmDenseRow row = rows[w.row];
		const AcmResampleRow r = rs[w.row];
		const bool converts = (row.count >> ACM_DENSE_MODE_SHIFT) != 0;
		const uint64_t count = row.count & ACM_DENSE_COUNT_MASK;
		const int16_t *from = src + row.src;
		OUT *o = out + w.row * row_len + (uint64_t)w.plane * sub_len;
		if (r.L != 0) {
			__syncthreads();                                /* the work before this one has read its table and planes */
			filtered_sub_row<OUT, LAYOUT, false>(from, converts, w.plane, r, taps, o, sub_len, w.unit, units, tab, xs);
		} else {
			plain_sub_row<OUT, LAYOUT>(from, converts, count, w.plane, o, sub_len, w.unit, units);
		}
	}
}

} // namespace

extern "C" int acmk_launch_dense_resample(const int16_t *d_src, const AcmDenseRow *d_rows, const AcmResampleRow *d_rs, const int16_t *d_taps,
					  uint64_t nrows, void *d_out, uint64_t frames, uint32_t channels, int planar, int f32, uint32_t dense_grid, void *stream)
{
	if (nrows == 0)
		return 0;
	const DenseGeo g = dense_geo(nrows, frames, channels, planar, dense_grid, DENSE_MAX_GRID);
	if (!g.ok)
		return (int)hipErrorInvalidValue;
	return dense_dispatch(f32, g.layout, [&](auto o, auto layout) {
		using OUT = decltype(o);
		hipLaunchKernelGGL((acm_dense_resample<OUT, decltype(layout)::value>), dim3(g.grid), dim3(DENSE_BLOCK), 0, (hipStream_t)stream, d_src,
				   d_rows, d_rs, d_taps, g.nwork, g.units, static_cast<OUT *>(d_out), g.row_len, g.sub_len);
		return (int)hipGetLastError();
	});
}
