/*
 * acm_overlay_layout.cpp - the device-free half of acm_batch_decode_windows_overlay (acm_batch_windows.cpp): the row table's
 * validation, the combine kernel's records, the list of source rows whose energy some row needs, and the sizes of the source arena and
 * of the device tables.  No HIP call here.
 */
#include "acm_overlay_layout.h"

namespace acmbatch {

int acm_overlay_prepare(const acm_overlay_row *rows, size_t nrows, size_t nwin, uint64_t row_words, uint64_t d_pcm_words, OverlayLayout *out)
{
	OverlayLayout &O = *out;
	O = OverlayLayout();
	if ((nrows && !rows) || row_words == 0 || row_words >= ACM_OVERLAY_MAX_ROW_WORDS)
		return ACMHIP_ERR_ARG;
	/* source rows are named by 32 bits, and ACM_OVERLAY_NONE is none of them */
	if (nwin > ACM_OVERLAY_NONE || (nrows && row_words > ~0ull / nrows) || d_pcm_words < nrows * row_words)
		return ACMHIP_ERR_ARG;
	for (size_t r = 0; r < nrows; r++) {
		const acm_overlay_row &w = rows[r];
		if (w.a >= nwin || (w.b != ACM_OVERLAY_NONE && w.b >= nwin) || w.reserved != 0 || w.vol > 65535)
			return ACMHIP_ERR_ARG;
		if (w.b != ACM_OVERLAY_NONE && w.snr == 0 && w.gain > ACM_OVERLAY_G_MAX)
			return ACMHIP_ERR_ARG;
	}
	O.row_words = row_words;
	O.nsrc = nwin;
	O.out_words = nrows * row_words;
	O.rows.resize(nrows);
	std::vector<uint8_t> need(nwin, 0);
	for (size_t r = 0; r < nrows; r++) {
		const acm_overlay_row &w = rows[r];
		const bool over = w.b != ACM_OVERLAY_NONE;
		O.rows[r] = AcmOverlayRow{ w.a, w.b, w.vol ? w.vol : 4096u, over ? w.snr : 0u, over && !w.snr ? w.gain : 0u, 0u };
		if (over && w.snr)
			need[w.a] = need[w.b] = 1;
	}
	for (size_t k = 0; k < nwin; k++)
		if (need[k])
			O.marked.push_back((uint32_t)k);
	return ACMHIP_OK;
}

void acm_overlay_report(const AcmOverlayResult &res, acm_overlay_row *row)
{
	row->gain = (uint32_t)res.gain;
	row->energy_a = res.energy_a;
	row->energy_b = res.energy_b;
}

} // namespace acmbatch

extern "C" uint32_t acm_dense_overlay_gain(uint64_t energy_a, uint64_t energy_b, uint32_t snr)
{
	return acm_overlay_gain(energy_a, energy_b, snr);
}

extern "C" int acmk_overlay_layout_visit(const acm_overlay_row *rows, size_t nrows, size_t nwin, uint64_t row_words, uint64_t d_pcm_words,
					 acmk_overlay_layout_visit_fn visit, void *ctx)
{
	using namespace acmbatch;
	OverlayLayout O;
	const int rc = acm_overlay_prepare(rows, nrows, nwin, row_words, d_pcm_words, &O);
	if (rc == ACMHIP_OK) {
		std::vector<uint64_t> rec, marked(O.marked.begin(), O.marked.end());
		for (const AcmOverlayRow &r : O.rows)
			rec.insert(rec.end(), { (uint64_t)r.a, (uint64_t)r.b, (uint64_t)r.vol, (uint64_t)r.snr, (uint64_t)r.gain });
		visit(ctx, "rows", rec.data(), 5 * sizeof(uint64_t), O.rows.size());
		visit(ctx, "marked", marked.data(), sizeof(uint64_t), marked.size());
	}
	const uint64_t totals[] = { (uint64_t)(int64_t)rc,  O.row_words,    O.out_words,     O.src_arena_words(), O.upload_bytes(),
				    O.energy_off(),        O.energy_bytes(), O.result_off(), O.result_bytes(),    O.table_bytes() };
	visit(ctx, "totals", totals, sizeof(uint64_t), sizeof(totals) / sizeof(totals[0]));
	return rc;
}
