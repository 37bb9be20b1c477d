// The launch geometry of the dense kernels under AddressSanitizer + UBSan (tests/test_dense_geo.py builds and runs this): dense_geo of
// acm_dense_geo.h - the one function all five launchers take their numbers from - against a table worked out by hand.  Nothing here
// knows a device.
#include <stdint.h>
#include <stdio.h>

#include "acm_dense_geo.h"

using namespace acm_dense;

static const uint32_t MOST = ACM_CAP_DENSE_GRID;

static int failures = 0;

#define CHECK(c)                                                                \
	do {                                                                    \
		if (!(c)) {                                                     \
			fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
			failures++;                                             \
		}                                                               \
	} while (0)

struct Case {
	uint64_t nrows, frames;
	uint32_t channels;
	int planar;
	uint32_t cap;
	bool whole_units;
	/* by hand */
	int layout;
	uint32_t subs;
	uint64_t row_len, sub_len;
	uint32_t units;
	uint64_t nwork;
	uint32_t grid;
};

static const Case CASES[] = {
	/* a unit is 256 lanes of 8 samples; the samples behind the last whole vector go with the last unit, and there is always one */
	{ 3, 0, 1, 0, 0, false, MONO, 1, 0, 0, 1, 3, 3 },
	{ 3, 7, 1, 0, 0, false, MONO, 1, 7, 7, 1, 3, 3 },
	{ 3, 8, 1, 0, 0, false, MONO, 1, 8, 8, 1, 3, 3 },
	{ 3, 2047, 1, 0, 0, false, MONO, 1, 2047, 2047, 1, 3, 3 },
	{ 3, 2048, 1, 0, 0, false, MONO, 1, 2048, 2048, 1, 3, 3 },
	{ 3, 2055, 1, 0, 0, false, MONO, 1, 2055, 2055, 1, 3, 3 },             /* 256 vectors and a tail of 7 */
	{ 3, 2056, 1, 0, 0, false, MONO, 1, 2056, 2056, 2, 6, 6 },             /* 257 vectors */
	{ 5, 4096 + 8, 1, 0, 0, false, MONO, 1, 4104, 4104, 3, 15, 15 },
	/* interleaved stereo: one sub-row of 2 T samples; planar: two of T, twice the work items of the mono batch */
	{ 3, 1028, 2, 0, 0, false, INTER, 1, 2056, 2056, 2, 6, 6 },
	{ 3, 1028, 2, 1, 0, false, PLANAR, 2, 2056, 1028, 1, 6, 6 },
	{ 3, 2056, 2, 1, 0, false, PLANAR, 2, 4112, 2056, 2, 12, 12 },
	{ 3, 2056, 1, 1, 0, false, MONO, 1, 2056, 2056, 2, 6, 6 },             /* planar means nothing to one channel */
	/* the energy launch: every sample is in a vector, so a unit is 2048 samples and no more */
	{ 4, 1, 1, 0, 0, true, MONO, 1, 1, 1, 1, 4, 4 },
	{ 4, 2048, 1, 0, 0, true, MONO, 1, 2048, 2048, 1, 4, 4 },
	{ 4, 2049, 1, 0, 0, true, MONO, 1, 2049, 2049, 2, 8, 8 },
	{ 4, 2055, 1, 0, 0, true, MONO, 1, 2055, 2055, 2, 8, 8 },              /* two units here, one in the gather */
	{ 4, 4096, 1, 0, 0, true, MONO, 1, 4096, 4096, 2, 8, 8 },
	{ 4, 4097, 1, 0, 0, true, MONO, 1, 4097, 4097, 3, 12, 12 },
	/* the cap: 0 is the built-in 2^20, 1 to 3 hold, nothing raises it, and a grid is never larger than the work */
	{ 7, 2056, 1, 0, 1, false, MONO, 1, 2056, 2056, 2, 14, 1 },
	{ 7, 2056, 1, 0, 2, false, MONO, 1, 2056, 2056, 2, 14, 2 },
	{ 7, 2056, 1, 0, 3, false, MONO, 1, 2056, 2056, 2, 14, 3 },
	{ 7, 2056, 1, 0, 100, false, MONO, 1, 2056, 2056, 2, 14, 14 },
	{ (1u << 20) + 7, 8, 1, 0, 0, false, MONO, 1, 8, 8, 1, (1u << 20) + 7, 1u << 20 },
	{ (1u << 20) + 7, 8, 1, 0, 1u << 20, false, MONO, 1, 8, 8, 1, (1u << 20) + 7, 1u << 20 },
	{ (1u << 20) + 7, 8, 1, 0, (1u << 20) + 1, false, MONO, 1, 8, 8, 1, (1u << 20) + 7, 1u << 20 },
	{ (1u << 20) + 7, 8, 1, 0, 0xFFFFFFFFu, false, MONO, 1, 8, 8, 1, (1u << 20) + 7, 1u << 20 },
	{ (1u << 20) + 7, 8, 1, 0, (1u << 20) - 1, false, MONO, 1, 8, 8, 1, (1u << 20) + 7, (1u << 20) - 1 },
	{ 3, 8, 1, 0, 0, true, MONO, 1, 8, 8, 1, 3, 3 },
	/* the largest sub-row: 2^31 - 1 units of 2048 samples */
	{ 2, 0x7FFFFFFFull * 2048, 1, 0, 0, false, MONO, 1, 0x7FFFFFFFull * 2048, 0x7FFFFFFFull * 2048, 0x7FFFFFFFu, 0xFFFFFFFEull, 1u << 20 },
	{ 2, 0x7FFFFFFFull * 2048 + 7, 1, 0, 0, false, MONO, 1, 0x7FFFFFFFull * 2048 + 7, 0x7FFFFFFFull * 2048 + 7, 0x7FFFFFFFu, 0xFFFFFFFEull, 1u << 20 },
	/* the most rows: nrows * units * subs = 2^64 - 1, and 2^64 - 2 with two sub-rows */
	{ ~0ull, 8, 1, 0, 0, false, MONO, 1, 8, 8, 1, ~0ull, 1u << 20 },
	{ ~0ull / 2, 8, 2, 1, 0, false, PLANAR, 2, 16, 8, 1, ~0ull - 1, 1u << 20 },
	{ ~0ull / 6, 2056, 2, 1, 0, false, PLANAR, 2, 4112, 2056, 2, ~0ull / 6 * 4, 1u << 20 },
};

int main()
{
	for (const Case &c : CASES) {
		const DenseGeo g = dense_geo(c.nrows, c.frames, c.channels, c.planar, c.cap, MOST, c.whole_units);
		const bool same = g.ok && g.layout == c.layout && g.subs == c.subs && g.row_len == c.row_len && g.sub_len == c.sub_len && g.units == c.units &&
				  g.nwork == c.nwork && g.grid == c.grid;
		if (!same) {
			fprintf(stderr, "nrows %llu frames %llu channels %u planar %d cap %u whole %d: ok %d layout %d subs %u row_len %llu sub_len %llu units %u "
				"nwork %llu grid %u\n", (unsigned long long)c.nrows, (unsigned long long)c.frames, c.channels, c.planar, c.cap, (int)c.whole_units,
				(int)g.ok, g.layout, g.subs, (unsigned long long)g.row_len, (unsigned long long)g.sub_len, g.units, (unsigned long long)g.nwork, g.grid);
			failures++;
		}
	}
	/* the two refusals.  Units past 2^31 - 1: one more vector than the largest sub-row has - in the gather a whole vector, in the energy
	 * launch a single sample */
	CHECK(!dense_geo(1, 0x7FFFFFFFull * 2048 + 8, 1, 0, 0, MOST).ok);
	CHECK(dense_geo(1, 0x7FFFFFFFull * 2048 + 7, 1, 0, 0, MOST).ok);
	CHECK(!dense_geo(1, 0x7FFFFFFFull * 2048 + 1, 1, 0, 0, MOST, true).ok);
	CHECK(dense_geo(1, 0x7FFFFFFFull * 2048, 1, 0, 0, MOST, true).ok);
	CHECK(!dense_geo(1, 0x7FFFFFFFull * 2048 + 8, 2, 1, 0, MOST).ok);              /* ... of a plane */
	CHECK(!dense_geo(1, 1ull << 62, 1, 0, 0, MOST).ok);
	/* nrows * units * subs past 2^64 */
	CHECK(!dense_geo(~0ull / 2 + 1, 8, 2, 1, 0, MOST).ok);                          /* 2^63 rows of two planes */
	CHECK(dense_geo(~0ull / 2 + 1, 8, 2, 0, 0, MOST).ok);                           /* ... of one sub-row */
	CHECK(!dense_geo(~0ull / 2 + 1, 2056, 1, 0, 0, MOST).ok);                       /* ... of two units */
	CHECK(!dense_geo(~0ull / 4 + 1, 2056, 2, 1, 0, MOST).ok && dense_geo(~0ull / 4, 2056, 2, 1, 0, MOST).ok);
	CHECK(!dense_geo(1ull << 34, 0x7FFFFFFFull * 2048, 1, 0, 0, MOST).ok && dense_geo(1ull << 33, 0x7FFFFFFFull * 2048, 1, 0, 0, MOST).ok);
	/* a refused launch has no work and no grid */
	const DenseGeo r = dense_geo(~0ull, 2056, 1, 0, 3, MOST);
	CHECK(!r.ok && r.nwork == 0 && r.grid == 0);
	/* no rows: no work (the launchers return before they ask) */
	const DenseGeo z = dense_geo(0, 2056, 2, 1, 0, MOST);
	CHECK(z.ok && z.units == 2 && z.subs == 2 && z.nwork == 0 && z.grid == 0);
	if (failures)
		return 1;
	printf("dense_geo: %zu cases\n", sizeof(CASES) / sizeof(CASES[0]));
	return 0;
}
