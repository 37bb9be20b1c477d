/*
 * acm_dense_call.h - one call of the dense family (acm_batch_decode_windows_dense, _overlay, _overlay_fir, _features, _logmel) described
 * without a device: what the caller asked for (DenseAsk), the layouts of its parts in the order the entry points refuse in
 * (acm_dense_call), where their tables sit in the H_JOBS / D_JOBS arenas (acm_jobs_map - the `base` the layout headers speak of),
 * and the bytes that go up (DenseCall::pack).  Internal.  Nothing here knows a device (tests/test_dense_call.py,
 * tests/native/dense_call.cpp); acm_batch_windows.cpp drives the device over a DenseCall it only reads.
 */
#ifndef ACM_DENSE_CALL_H
#define ACM_DENSE_CALL_H

#include <string.h>

#include "acm_dense_layout.h"
#include "acm_feat_layout.h"
#include "acm_fir_layout.h"
#include "acm_overlay_layout.h"

namespace acmbatch {

/* what an entry point was called with, beyond the windowed decode's own arguments */
enum DenseKind {
	DENSE_ROWS = 0,         /* acm_batch_decode_windows_dense: opts->d_pcm receives a row per window */
	DENSE_OVERLAY = 1,      /* ..._overlay, ..._overlay_fir: the windows are the sources of the nrows rows of `rows`, which it receives */
	DENSE_FEATURES = 2,     /* ..._features: those rows go to the feature arena, int16, and it receives `bank`'s features of them */
};
struct DenseAsk {
	DenseKind kind;
	const acm_dense_opts *dense;
	acm_overlay_row *rows;          /* DENSE_ROWS: null */
	size_t nrows;
	const acm_fir_opts *fir;        /* the responses, or null */
	const acm_feat_bank *bank;      /* DENSE_FEATURES: the bank (a null one is refused); else null */
	const acm_feat_log *log = nullptr;      /* DENSE_FEATURES of acm_batch_decode_windows_logmel: the scale; else null */
};

/* The H_JOBS / D_JOBS arenas of a dense call: the device parser's tables and results (WindowLayout::job_arena_bytes()), behind them
 * the dense tables, the overlay's, the filter pass's taps and rows, the bank's - each from a multiple of 64 on, in that order.  A
 * section a call does not have is ACM_JOBS_NONE bytes long (a filter section of 0 bytes is none either): it takes no room, and its
 * offset is where it would begin.  total: the end of the last section the call has */
constexpr size_t ACM_JOBS_NONE = ~(size_t)0;
struct JobsMap {
	size_t dense, overlay, fir, feat, total;
};
inline JobsMap acm_jobs_map(size_t parser_bytes, size_t dense_bytes, size_t overlay_bytes, size_t fir_bytes, size_t feat_bytes)
{
	size_t end = parser_bytes;
	auto place = [&end](size_t bytes) {
		const size_t at = (size_t)round_up(end, 64);
		if (bytes != ACM_JOBS_NONE)
			end = at + bytes;
		return at;
	};
	JobsMap m{};
	m.dense = place(dense_bytes);
	m.overlay = place(overlay_bytes);
	m.fir = place(fir_bytes ? fir_bytes : ACM_JOBS_NONE);
	m.feat = place(feat_bytes);
	m.total = end;
	return m;
}
inline size_t DenseLayout::table_off(const WindowLayout &L) const { return acm_jobs_map(L.job_arena_bytes(), 0, ACM_JOBS_NONE, 0, ACM_JOBS_NONE).dense; }

/* a piece of H_JOBS that goes up to the same place of D_JOBS */
struct JobsSpan {
	size_t off, bytes;
};
struct DensePacked {
	DenseLaunch gather;     /* which kernel takes the gather launch (acm_dense_layout.cpp) */
	JobsSpan span[4];       /* the dense tables, the overlay's rows and list, the filter's tables, the bank's: those the call has */
	size_t nspan;
};

struct DenseCall {
	DenseKind kind = DENSE_ROWS;
	DenseLayout D;
	OverlayLayout O;        /* overlay(): an overlay call - a dense call whose rows go to the source arena */
	FirLayout F;            /* fir(): ... some of whose windows are filtered */
	FeatLayout M;           /* feat(): ... whose rows go to the feature arena and are framed there */
	JobsMap map{};          /* place() */
	const OverlayLayout *overlay() const { return kind != DENSE_ROWS ? &O : nullptr; }
	const FirLayout *fir() const { return F.nfilt() ? &F : nullptr; }     /* a filter call without a filtered window is an overlay call */
	const FeatLayout *feat() const { return kind == DENSE_FEATURES ? &M : nullptr; }
	/* once the window layout underneath (over D.wins and D.inner) says how long the parser's part of the arenas is */
	void place(size_t parser_bytes)
	{
		map = acm_jobs_map(parser_bytes, D.table_bytes(), overlay() ? O.table_bytes() : ACM_JOBS_NONE, F.table_bytes(), feat() ? M.table_bytes() : ACM_JOBS_NONE);
	}
	/* every table that goes up, written into h_jobs (map.total bytes) by what staging left of every window (final[k].words, as
	 * acm_dense_tables takes it: it decides the kernel and how much of the dense tables it reads), and the spans of it to upload:
	 * nothing outside them is written */
	DensePacked pack(uint8_t *h_jobs, const WindowSlot *slots, const acm_batch_window *final) const
	{
		DensePacked p{};
		p.gather = acm_dense_tables(D, slots, final, h_jobs + map.dense);
		p.span[p.nspan++] = JobsSpan{ map.dense, p.gather.bytes };
		if (overlay() && O.upload_bytes()) {
			memcpy(h_jobs + map.overlay, O.rows.data(), O.rows_bytes());
			memcpy(h_jobs + map.overlay + O.marked_off(), O.marked.data(), O.marked.size() * sizeof(uint32_t));
			p.span[p.nspan++] = JobsSpan{ map.overlay, O.upload_bytes() };
		}
		if (fir()) {
			memcpy(h_jobs + map.fir, F.taps.data(), F.taps_bytes());
			memcpy(h_jobs + map.fir + F.rows_off(), F.rows.data(), F.rows.size() * sizeof(AcmFirRow));
			p.span[p.nspan++] = JobsSpan{ map.fir, F.table_bytes() };
		}
		if (feat()) {
			M.pack(h_jobs + map.feat);
			p.span[p.nspan++] = JobsSpan{ map.feat, M.table_bytes() };
		}
		return p;
	}
};

/* The four prepare calls and acm_fir_remap over one call's arguments; opts: the caller's, defaults filled in.  ACMHIP_OK, or
 * ACMHIP_ERR_ARG with *why the error text of the first part that refuses - then nothing of `out` is to be used */
inline int acm_dense_call(const WindowItem *items, size_t n, const acm_batch_window *wins, size_t nwin, const acm_batch_opts &opts,
			  const DenseAsk &ask, DenseCall *out, const char **why)
{
	DenseCall &c = *out;
	c = DenseCall();
	c.kind = ask.kind;
	const bool overlay = ask.kind != DENSE_ROWS, feat = ask.kind == DENSE_FEATURES;
	/* the room behind d_pcm is measured against the output rows of an overlay call, by its own layout */
	acm_batch_opts asked = opts;
	if (overlay)
		asked.d_pcm_words = ~0ull;
	*why = "acm_batch_decode_windows_dense: a call the dense writer does not take (include/acm_hip.h)";
	if (acm_dense_prepare(items, n, wins, nwin, asked, ask.dense, &c.D) != ACMHIP_OK)
		return ACMHIP_ERR_ARG;
	/* ... and of a features call against the features of those rows, by its own layout again */
	*why = "acm_batch_decode_windows_overlay: a row table the call does not take (include/acm_hip.h)";
	if (overlay && acm_overlay_prepare(ask.rows, ask.nrows, nwin, c.D.row_words, feat ? ~0ull : opts.d_pcm_words, &c.O) != ACMHIP_OK)
		return ACMHIP_ERR_ARG;
	*why = "acm_batch_decode_windows_overlay_fir: responses the call does not take (include/acm_hip.h)";
	if (overlay && ask.fir) {
		if (acm_fir_prepare(ask.fir, nwin, &c.F) != ACMHIP_OK)
			return ACMHIP_ERR_ARG;
		acm_fir_remap(c.F, &c.O);
	}
	*why = "acm_batch_decode_windows_features: a bank or a tensor the call does not take (include/acm_hip.h)";
	if (feat && !ask.log && acm_feat_prepare(ask.bank, ask.dense->channels, c.D.frames, ask.nrows, opts.d_pcm_words, &c.M) != ACMHIP_OK)
		return ACMHIP_ERR_ARG;
	*why = "acm_batch_decode_windows_logmel: a bank, a scale or a tensor the call does not take (include/acm_hip.h)";
	if (feat && ask.log && acm_feat_prepare(ask.bank, ask.log, ask.dense->channels, c.D.frames, ask.nrows, opts.d_pcm_words, &c.M) != ACMHIP_OK)
		return ACMHIP_ERR_ARG;
	*why = nullptr;
	return ACMHIP_OK;
}

} // namespace acmbatch

#endif
