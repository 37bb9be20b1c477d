/*
 * acm_dense_speed.hip - acm_dense_resample.hip's gather for a call with ACM_DENSE_SPEED (include/acm_hip.h) in which some row takes
 * the wide filter: a window played at a speed of its own, or a file at a rate whose exact polyphase table would not fit LDS.  Such a
 * row is filtered between two neighbouring phases of its cutoff's prototype table, at a position stepped in 32.32 fixed point; the
 * rows of the exact filter, the converting and the plain rows are written as acm_dense_resample writes them.  Launched only where the
 * second row table says that a row is wide (acm_dense_layout.cpp); every other call keeps the kernel it had.
 *
 * No counterpart in the reference.  The geometry is acm_dense_resample's and the code of a unit and of the loop is shared with it
 * (acm_dense_filter.h): the table - P + 1 phases, (P + 1) * K <= 16384 taps - and the converted source span in 63 KB of LDS, passes
 * that halve where a span outgrows the planes (sized by the fixed-point bases), one 64-bit multiply a lane and the step from there, a
 * source sample read once for both sums, no scratch, no float before the final times 2^-15.  A workgroup works on one row, so the
 * filter's form is a workgroup-uniform branch.
 */
#include <hip/hip_runtime.h>

#include "acm_dense_filter.h"

namespace {

/* sub_len: output samples of a sub-row (frames with PLANAR, else the whole row); units: workgroups per sub-row */
template <typename OUT, int LAYOUT>
__global__ __launch_bounds__(DENSE_BLOCK) void acm_dense_speed(const int16_t *__restrict__ src, const AcmDenseRow *__restrict__ rows,
								const AcmSpeedRow *__restrict__ sp, const int16_t *__restrict__ taps, uint64_t nwork,
								uint32_t units, OUT *__restrict__ out, uint64_t row_len, uint64_t sub_len)
{
	__shared__ __attribute__((aligned(16))) int16_t tab[TAB_CAP];
	__shared__ __attribute__((aligned(16))) int16_t xs[SPAN_CAP];
	for (uint64_t work = blockIdx.x; work < nwork; work += gridDim.x) {
		const WorkItem w = work_item<LAYOUT == PLANAR ? 2 : 1>(work, units);
		const AcmDenseRow row = rows[w.row];
		const AcmSpeedRow r = sp[w.row];
		const bool converts = (row.count >> ACM_DENSE_MODE_SHIFT) != 0;
		const uint64_t count = row.count & ACM_DENSE_COUNT_MASK;
		const int16_t *from = src + row.src;
		OUT *o = out + w.row * row_len + (uint64_t)w.plane * sub_len;
		if (r.L != 0) {
			__syncthreads();                                /* the work before this one has read its table and planes */
			if (r.wide)
				filtered_sub_row<OUT, LAYOUT, true>(from, converts, w.plane, r, taps, o, sub_len, w.unit, units, tab, xs);
			else
				filtered_sub_row<OUT, LAYOUT, false>(from, converts, w.plane, r, taps, o, sub_len, w.unit, units, tab, xs);
		} else {
			plain_sub_row<OUT, LAYOUT>(from, converts, count, w.plane, o, sub_len, w.unit, units);
		}
	}
}

} // namespace

extern "C" int acmk_launch_dense_speed(const int16_t *d_src, const AcmDenseRow *d_rows, const AcmSpeedRow *d_sp, const int16_t *d_taps,
				       uint64_t nrows, void *d_out, uint64_t frames, uint32_t channels, int planar, int f32, uint32_t dense_grid, void *stream)
{
	if (nrows == 0)
		return 0;
	const DenseGeo g = dense_geo(nrows, frames, channels, planar, dense_grid, DENSE_MAX_GRID);
	if (!g.ok)
		return (int)hipErrorInvalidValue;
	return dense_dispatch(f32, g.layout, [&](auto o, auto layout) {
		using OUT = decltype(o);
		hipLaunchKernelGGL((acm_dense_speed<OUT, decltype(layout)::value>), dim3(g.grid), dim3(DENSE_BLOCK), 0, (hipStream_t)stream, d_src, d_rows,
				   d_sp, d_taps, g.nwork, g.units, static_cast<OUT *>(d_out), g.row_len, g.sub_len);
		return (int)hipGetLastError();
	});
}
