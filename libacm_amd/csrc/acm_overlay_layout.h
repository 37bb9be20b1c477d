/*
 * acm_overlay_layout.h - the device-free half of acm_batch_decode_windows_overlay (acm_batch_windows.cpp): whether the row table is one
 * the call takes, which source rows need an energy, how large the source arena and the device tables are - and the one text of the
 * gain formula, which the combine kernel (acm_dense_overlay.hip) and acm_dense_overlay_gain both compile.  Internal.  Neither this
 * header nor acm_overlay_layout.cpp knows a device (tests/test_dense_overlay.py); the source rows themselves are the dense call's,
 * validated and laid out by acm_dense_layout.cpp as ever.
 */
#ifndef ACM_OVERLAY_LAYOUT_H
#define ACM_OVERLAY_LAYOUT_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "acm_device.h"

#ifdef __HIP__
#define ACM_OVERLAY_HD __host__ __device__
#else
#define ACM_OVERLAY_HD
#endif

#define ACM_OVERLAY_G_MAX 32768u
#define ACM_OVERLAY_MAX_ROW_WORDS (1ull << 24)          /* R below it: Ea << 40 stays below 2^94, g^2 * D below 2^116 */

/* g of include/acm_hip.h: min(G_MAX, isqrt((Ea << 40) / (Eb * snr))), 0 where Eb * snr == 0.  g^2 <= N / D is g^2 * D <= N on
 * integers, so the largest such g is found bit by bit and nothing is divided: 16 products of 128 bits */
ACM_OVERLAY_HD static inline uint32_t acm_overlay_gain(uint64_t energy_a, uint64_t energy_b, uint32_t snr)
{
	const unsigned __int128 D = (unsigned __int128)energy_b * snr, N = (unsigned __int128)energy_a << 40;
	if (D == 0)
		return 0;
	if ((unsigned __int128)((uint64_t)ACM_OVERLAY_G_MAX * ACM_OVERLAY_G_MAX) * D <= N)
		return ACM_OVERLAY_G_MAX;
	uint32_t g = 0;
	for (uint32_t bit = ACM_OVERLAY_G_MAX >> 1; bit; bit >>= 1) {
		const uint32_t t = g | bit;
		if ((unsigned __int128)((uint64_t)t * t) * D <= N)
			g = t;
	}
	return g;
}

namespace acmbatch {

/* samples the source arena is asked for beyond the source rows: the kernels load only aligned 16-byte lines that hold a sample of
 * the row they read, so at most 7 samples behind the last row; the dense call's own slack keeps that inside memory the call owns */
constexpr uint64_t ACM_OVERLAY_SRC_SLACK = 64;

struct OverlayLayout {
	uint64_t row_words = 0;                 /* R */
	size_t nsrc = 0;                        /* source rows: the call's windows */
	uint64_t out_words = 0;                 /* nrows * R: what opts->d_pcm must hold */
	std::vector<AcmOverlayRow> rows;        /* the combine kernel's table, one record per output row; vol 0 is 4096 here */
	std::vector<uint32_t> marked;           /* the source rows some row in SNR mode names, ascending, each once: the energy launch's list */
	uint64_t src_arena_words() const { return nsrc * row_words + ACM_OVERLAY_SRC_SLACK; }
	/* the tables travel behind the dense call's in the H_JOBS / D_JOBS arenas, from `base` (a multiple of 64) on: the row table and
	 * the list go up; the energies (one per SOURCE row, zeroed by the call) and the row results stay on the device, and the results
	 * come back to the same place of H_JOBS */
	size_t rows_bytes() const { return rows.size() * sizeof(AcmOverlayRow); }
	size_t marked_off() const { return rows_bytes(); }
	size_t upload_bytes() const { return (marked_off() + marked.size() * sizeof(uint32_t) + 7) / 8 * 8; }
	size_t energy_off() const { return upload_bytes(); }
	size_t energy_bytes() const { return nsrc * sizeof(uint64_t); }
	size_t result_off() const { return energy_off() + energy_bytes(); }
	size_t result_bytes() const { return rows.size() * sizeof(AcmOverlayResult); }
	size_t table_bytes() const { return result_off() + result_bytes(); }
};

/* ACMHIP_OK, or ACMHIP_ERR_ARG for a row table the call refuses (include/acm_hip.h) - then nothing of `out` is to be used.
 * row_words: R of the dense options the call came with, d_pcm_words: the room behind opts->d_pcm */
int acm_overlay_prepare(const acm_overlay_row *rows, size_t nrows, size_t nwin, uint64_t row_words, uint64_t d_pcm_words, OverlayLayout *out);

/* what the caller's row r receives, from the result the combine kernel left for it */
void acm_overlay_report(const AcmOverlayResult &res, acm_overlay_row *row);

} // namespace acmbatch

extern "C" {
typedef void (*acmk_overlay_layout_visit_fn)(void *ctx, const char *name, const void *data, size_t elem_bytes, size_t count);
/* The overlay layout shown to a visitor (tests).  A refused table visits "totals" alone.  Tables, as uint64 words: "rows" (5 per
 * output row: a, b, vol, snr, gain as the kernel gets them), "marked" (1 per source row that gets an energy), "totals": the return
 * code, row_words, out_words, src_arena_words, upload_bytes, energy_off, energy_bytes, result_off, result_bytes, table_bytes */
int acmk_overlay_layout_visit(const acm_overlay_row *rows, size_t nrows, size_t nwin, uint64_t row_words, uint64_t d_pcm_words,
			      acmk_overlay_layout_visit_fn visit, void *ctx);
}

#endif
