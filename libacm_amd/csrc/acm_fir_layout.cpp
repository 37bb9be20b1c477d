/*
 * acm_fir_layout.cpp - the device-free half of acm_batch_decode_windows_overlay_fir (acm_batch_windows.cpp): the responses' validation
 * (acm_dense_fir_check, the one text of it), the list of filtered windows, the packed taps, and the overlay layout rewritten to name
 * the filtered rows.  No HIP call here.
 */
#include "acm_fir_layout.h"

#include <unordered_map>

extern "C" int acm_dense_fir_check(const acm_fir_response *r)
{
	if (!r || !r->taps || r->ntaps == 0 || r->ntaps > ACM_FIR_MAX_TAPS || r->delay >= r->ntaps || r->shift > ACM_FIR_MAX_SHIFT || r->reserved != 0)
		return ACMHIP_ERR_ARG;
	uint64_t l1 = 0;
	for (uint32_t t = 0; t < r->ntaps; t++)
		l1 += (uint64_t)(r->taps[t] < 0 ? -(int)r->taps[t] : (int)r->taps[t]);
	return l1 <= ACM_FIR_MAX_L1 ? ACMHIP_OK : ACMHIP_ERR_ARG;
}

namespace acmbatch {

int acm_fir_prepare(const acm_fir_opts *fir, size_t nwin, FirLayout *out)
{
	FirLayout &F = *out;
	F = FirLayout();
	F.nwin = nwin;
	F.slot.resize(nwin);
	for (size_t k = 0; k < nwin; k++)
		F.slot[k] = (uint32_t)k;
	if (!fir || fir->nresp == 0)
		return ACMHIP_OK;
	if (!fir->responses || !fir->of_window || fir->nresp > ACM_FIR_MAX_RESPONSES || fir->reserved != 0)
		return ACMHIP_ERR_ARG;
	size_t nfilt = 0;
	for (size_t k = 0; k < nwin; k++) {
		if (fir->of_window[k] != ACM_FIR_NONE && fir->of_window[k] >= fir->nresp)
			return ACMHIP_ERR_ARG;
		nfilt += fir->of_window[k] != ACM_FIR_NONE;
	}
	if ((uint64_t)nwin + nfilt >= ACM_OVERLAY_NONE)         /* arena rows are named by 32 bits */
		return ACMHIP_ERR_ARG;
	for (size_t p = 0; p < fir->nresp; p++)
		if (acm_dense_fir_check(&fir->responses[p]) != ACMHIP_OK)
			return ACMHIP_ERR_ARG;
	/* the responses some window names, each packed once, in the order the windows come to them */
	std::unordered_map<uint32_t, AcmFirRow> packed;
	uint64_t named_taps = 0;
	for (size_t k = 0; k < nwin; k++) {
		const uint32_t p = fir->of_window[k];
		if (p == ACM_FIR_NONE)
			continue;
		auto it = packed.find(p);
		if (it == packed.end()) {
			const acm_fir_response &r = fir->responses[p];
			named_taps += r.ntaps;
			if (named_taps > ACM_FIR_MAX_CALL_TAPS)
				return ACMHIP_ERR_ARG;
			/* g[u] = h[ntaps - 1 - u], zeros behind: y[j] = sum over u of g[u] * x[j + lead + u], both operands read upwards */
			const uint32_t nblk = (r.ntaps + ACM_FIR_TAP_BLOCK - 1) / ACM_FIR_TAP_BLOCK;
			const size_t at = F.taps.size();
			F.taps.resize(at + (size_t)nblk * ACM_FIR_TAP_BLOCK, 0);
			for (uint32_t u = 0; u < r.ntaps; u++)
				F.taps[at + u] = r.taps[r.ntaps - 1 - u];
			AcmFirRow rec{};
			rec.taps_off = (uint32_t)(at / 2);
			rec.nblk = nblk;
			rec.lead = (int32_t)r.delay - (int32_t)(r.ntaps - 1);
			rec.shift = r.shift;
			it = packed.emplace(p, rec).first;
		}
		AcmFirRow rec = it->second;
		rec.src = (uint32_t)k;
		rec.dst = (uint32_t)(nwin + F.rows.size());
		F.slot[k] = rec.dst;
		F.rows.push_back(rec);
	}
	return ACMHIP_OK;
}

void acm_fir_remap(const FirLayout &F, OverlayLayout *O)
{
	if (F.rows.empty())
		return;
	for (AcmOverlayRow &r : O->rows) {
		r.a = F.slot[r.a];
		if (r.b != ACM_OVERLAY_NONE)
			r.b = F.slot[r.b];
	}
	for (uint32_t &k : O->marked)
		k = F.slot[k];
	O->nsrc = F.nwin + F.rows.size();
}

} // namespace acmbatch

extern "C" int acmk_fir_layout_visit(const acm_overlay_row *rows, size_t nrows, size_t nwin, uint64_t row_words, uint64_t d_pcm_words,
				     const acm_fir_opts *fir, acmk_fir_layout_visit_fn visit, void *ctx)
{
	using namespace acmbatch;
	OverlayLayout O;
	FirLayout F;
	int rc = acm_overlay_prepare(rows, nrows, nwin, row_words, d_pcm_words, &O);
	if (rc == ACMHIP_OK)
		rc = acm_fir_prepare(fir, nwin, &F);
	if (rc == ACMHIP_OK) {
		acm_fir_remap(F, &O);
		std::vector<uint64_t> fr, slot(F.slot.begin(), F.slot.end()), rec, marked(O.marked.begin(), O.marked.end());
		for (const AcmFirRow &r : F.rows)
			fr.insert(fr.end(), { (uint64_t)r.src, (uint64_t)r.dst, (uint64_t)r.taps_off, (uint64_t)r.nblk, (uint64_t)(int64_t)r.lead, (uint64_t)r.shift });
		for (const AcmOverlayRow &r : O.rows)
			rec.insert(rec.end(), { (uint64_t)r.a, (uint64_t)r.b, (uint64_t)r.vol, (uint64_t)r.snr, (uint64_t)r.gain });
		visit(ctx, "fir_rows", fr.data(), 6 * sizeof(uint64_t), F.rows.size());
		visit(ctx, "slot", slot.data(), sizeof(uint64_t), slot.size());
		visit(ctx, "taps", F.taps.data(), sizeof(int16_t), F.taps.size());
		visit(ctx, "rows", rec.data(), 5 * sizeof(uint64_t), O.rows.size());
		visit(ctx, "marked", marked.data(), sizeof(uint64_t), marked.size());
	}
	const bool ok = rc == ACMHIP_OK;
	const uint64_t totals[] = { (uint64_t)(int64_t)rc,
				    ok ? F.nfilt() : 0,
				    ok ? F.taps_bytes() : 0,
				    ok ? F.rows_off() : 0,
				    ok ? F.table_bytes() : 0,
				    ok ? O.nsrc : 0,
				    ok ? O.src_arena_words() : 0,
				    ok ? O.energy_bytes() : 0,
				    ok ? O.table_bytes() : 0,
				    ACM_FIR_TAP_BLOCK };
	visit(ctx, "totals", totals, sizeof(uint64_t), sizeof(totals) / sizeof(totals[0]));
	return rc;
}
