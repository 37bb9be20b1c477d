/*
 * acm_dense_geo.h - the launch geometry of every dense kernel (acm_dense.hip, acm_dense_mix.hip, acm_dense_resample.hip,
 * acm_dense_speed.hip, acm_dense_overlay.hip), written once.  Plain C++ - no HIP header, nothing __device__ - so that the launchers
 * and a program without a device (tests/native/dense_geo.cpp) ask the same text.
 *
 * A row of the output is cut into sub-rows - one, or with PLANAR one per plane - and a sub-row into units: a workgroup of
 * DENSE_BLOCK lanes, a vector of DENSE_VEC output samples a lane.  The samples behind a sub-row's last whole vector go with its last
 * unit, so a sub-row shorter than a vector still has one.  The grid is flat over (row, sub-row, unit), capped, and the kernels stride
 * over what is left: work = blockIdx.x, += gridDim.x.
 */
#ifndef ACM_DENSE_GEO_H
#define ACM_DENSE_GEO_H

#include <stdint.h>

#include "acm_launch_caps.h"

namespace acm_dense {

constexpr int DENSE_BLOCK = 256;        /* lanes per workgroup = vectors per unit */
constexpr int DENSE_VEC = 8;            /* output samples per body access */
constexpr uint32_t DENSE_UNIT = DENSE_BLOCK * DENSE_VEC;       /* samples of a unit's vectors */

enum Layout { MONO = 0, INTER = 1, PLANAR = 2 };        /* of the batch: C = 1, C = 2 as [T][2], C = 2 as [2][T] */

struct DenseGeo {
	int layout;
	uint32_t subs;                  /* sub-rows per row */
	uint64_t row_len, sub_len;      /* output samples of a row, and of a sub-row (frames with PLANAR, else the whole row) */
	uint32_t units;                 /* workgroups per sub-row */
	uint64_t nwork;                 /* nrows * subs * units */
	uint32_t grid;
	bool ok;                        /* false: more work than the kernels' counters hold - the launcher's hipErrorInvalidValue */
};

/* nrows rows of frames * channels samples.  dense_grid: the handle's launch cap, 0 = `most`, the built-in one, which nothing raises.
 * whole_units (acm_dense_energy, which has no narrow accesses): a sub-row's last samples make a vector, and a unit, of their own */
inline DenseGeo dense_geo(uint64_t nrows, uint64_t frames, uint32_t channels, int planar, uint32_t dense_grid, uint32_t most,
			  bool whole_units = false)
{
	DenseGeo g{};
	g.layout = channels == 1 ? MONO : planar ? PLANAR : INTER;
	g.subs = g.layout == PLANAR ? 2 : 1;
	g.row_len = frames * channels;
	g.sub_len = g.subs == 2 ? frames : g.row_len;
	const uint64_t vecs = g.sub_len / DENSE_VEC + (whole_units && g.sub_len % DENSE_VEC != 0);
	const uint64_t units = vecs <= DENSE_BLOCK ? 1 : (vecs + DENSE_BLOCK - 1) / DENSE_BLOCK;
	g.ok = units <= 0x7FFFFFFFull && nrows <= ~0ull / (units * g.subs);
	g.units = (uint32_t)units;
	g.nwork = g.ok ? nrows * units * g.subs : 0;
	const uint32_t cap = acm_cap_value(dense_grid, most);
	g.grid = (uint32_t)(g.nwork < cap ? g.nwork : cap);
	return g;
}

} // namespace acm_dense

#endif
