/*
 * acm_dense_resample.hip - acm_dense_mix.hip's gather for a call with ACM_DENSE_RESAMPLE (include/acm_hip.h) in which some window's
 * file has another sample rate than the batch: the rows of such windows are filtered to the batch's rate on the way, the others are
 * laid out - copied, split, down- or up-mixed - as acm_dense_mixed lays them out.  Launched only where the second row table says that
 * a row is filtered (acm_dense_layout.cpp); every other call keeps the kernel it had.
 *
 * No counterpart in the reference.  The filter, the staging of a unit and the geometry - acm_dense_mixed's: sub-rows (one, or one
 * per plane), units of 256 lanes and 2048 outputs, a flat grid that strides over (row, sub-row, unit); a workgroup works on one row, so
 * its kind is a workgroup-uniform branch - are acm_dense_filter.h's, shared with acm_dense_speed.hip.
 */
#include <hip/hip_runtime.h>

#include "acm_dense_filter.h"

namespace {

/* sub_len: output samples of a sub-row (frames with PLANAR, else the whole row); units: workgroups per sub-row */
template <typename OUT, int LAYOUT>
__global__ __launch_bounds__(DENSE_BLOCK) void acm_dense_resample(const int16_t *__restrict__ src, const AcmDenseRow *__restrict__ rows,
								   const AcmResampleRow *__restrict__ rs, const int16_t *__restrict__ taps, uint64_t nwork,
								   uint32_t units, OUT *__restrict__ out, uint64_t row_len, uint64_t sub_len)
{
	__shared__ __attribute__((aligned(16))) int16_t tab[TAB_CAP];
	__shared__ __attribute__((aligned(16))) int16_t xs[SPAN_CAP];
	constexpr uint32_t SUBS = LAYOUT == PLANAR ? 2 : 1;
	const uint32_t per_row = units * SUBS;
	for (uint64_t work = blockIdx.x; work < nwork; work += gridDim.x) {
		const uint64_t k = work / per_row;
		const uint32_t rem = (uint32_t)(work - k * per_row);
		const uint32_t plane = SUBS == 2 ? rem / units : 0;
		const uint32_t unit = rem - plane * units;
		const AcmDenseRow row = rows[k];
		const AcmResampleRow r = rs[k];
		const bool converts = (row.count >> ACM_DENSE_MODE_SHIFT) != 0;
		const uint64_t count = row.count & ACM_DENSE_COUNT_MASK;
		const int16_t *from = src + row.src;
		OUT *o = out + k * row_len + (uint64_t)plane * sub_len;
		if (r.L != 0) {
			__syncthreads();                                /* the work before this one has read its table and planes */
			filtered_sub_row<OUT, LAYOUT, false>(from, converts, plane, r, taps, o, sub_len, unit, units, tab, xs);
		} else {
			plain_sub_row<OUT, LAYOUT>(from, converts, count, plane, o, sub_len, unit, units);
		}
	}
}

template <typename OUT, int LAYOUT>
int launch(const FilterGeo &g, hipStream_t st, const int16_t *d_src, const AcmDenseRow *d_rows, const AcmResampleRow *d_rs, const int16_t *d_taps,
	   void *d_out)
{
	hipLaunchKernelGGL((acm_dense_resample<OUT, LAYOUT>), dim3(g.grid), dim3(DENSE_BLOCK), 0, st, d_src, d_rows, d_rs, d_taps, g.nwork, g.units,
			   static_cast<OUT *>(d_out), g.row_len, g.sub_len);
	return (int)hipGetLastError();
}

} // namespace

extern "C" int acmk_launch_dense_resample(const int16_t *d_src, const AcmDenseRow *d_rows, const AcmResampleRow *d_rs, const int16_t *d_taps,
					  uint64_t nrows, void *d_out, uint64_t frames, uint32_t channels, int planar, int f32, uint32_t dense_grid, void *stream)
{
	if (nrows == 0)
		return 0;
	const FilterGeo g = filter_geo(nrows, frames, channels, planar, dense_grid);
	if (!g.ok)
		return (int)hipErrorInvalidValue;
	hipStream_t st = (hipStream_t)stream;
#define ACM_RS_LAUNCH(OUT, LAYOUT) launch<OUT, LAYOUT>(g, st, d_src, d_rows, d_rs, d_taps, d_out)
	if (f32)
		return g.layout == MONO ? ACM_RS_LAUNCH(float, MONO) : g.layout == INTER ? ACM_RS_LAUNCH(float, INTER) : ACM_RS_LAUNCH(float, PLANAR);
	return g.layout == MONO ? ACM_RS_LAUNCH(int16_t, MONO) : g.layout == INTER ? ACM_RS_LAUNCH(int16_t, INTER) : ACM_RS_LAUNCH(int16_t, PLANAR);
#undef ACM_RS_LAUNCH
}
