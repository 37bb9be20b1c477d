/*
 * acm_dense_layout.cpp - the device-free half of acm_batch_decode_windows_dense (acm_batch_windows.cpp): the call's validation, its
 * soft rejections, the output size and the gather kernel's row table - with ACM_DENSE_RESAMPLE also which windows are filtered by
 * which ratio's table (acm_resample_layout.cpp) and the second row table that says so, with ACM_DENSE_SPEED the windows' speeds, the
 * two forms of the filter and the larger records of a call with a wide row.  No HIP call here.
 */
#include "acm_dense_layout.h"

#include <string.h>

#include "acm_dense_call.h"     /* DenseLayout::table_off: the jobs-arena map */

namespace acmbatch {

int acm_dense_prepare(const WindowItem *items, size_t n, const acm_batch_window *wins, size_t nwin, const acm_batch_opts &opts,
		      const acm_dense_opts *dense, DenseLayout *out)
{
	DenseLayout &D = *out;
	D = DenseLayout();
	if (!dense || dense->frames == 0 || (dense->channels != 1 && dense->channels != 2) ||
	    (dense->flags & ~(ACM_DENSE_PLANAR | ACM_DENSE_MIX | ACM_DENSE_RESAMPLE | ACM_DENSE_SPEED)))
		return ACMHIP_ERR_ARG;
	/* the two fields behind `flags` exist for a caller that sets the flag; the products of frames and a ratio stay far inside 64 bits */
	D.resample = (dense->flags & ACM_DENSE_RESAMPLE) != 0;
	if (D.resample && (dense->rate == 0 || dense->reserved != 0 || dense->frames >= (1ull << 40)))
		return ACMHIP_ERR_ARG;
	D.rate = D.resample ? dense->rate : 0;
	/* a window's speed is read with its flag alone; an output frame's position is its number times a step below 2^36, in 64 bits */
	D.speed = (dense->flags & ACM_DENSE_SPEED) != 0;
	if (D.speed && (!D.resample || dense->frames >= (1ull << 28)))
		return ACMHIP_ERR_ARG;
	for (size_t k = 0; D.speed && k < nwin; k++)
		if (wins[k].reserved && (!(wins[k].reserved >> 16) || !(wins[k].reserved & 0xFFFF)))
			return ACMHIP_ERR_ARG;
	/* padding has one meaning in the signed little-endian writer only; the staged forms of a prestaged or packed batch are not a window's */
	if (!opts.d_pcm || opts.fmt != ACMHIP_FMT_S16LE || opts.parse > ACM_BATCH_PARSE_AUTO || opts.prestaged || (opts.flags & ACM_BATCH_STAGE_PACKED))
		return ACMHIP_ERR_ARG;
	if (dense->frames > ~0ull / dense->channels)
		return ACMHIP_ERR_ARG;
	D.frames = dense->frames;
	D.channels = dense->channels;
	D.row_words = D.frames * D.channels;
	D.planar = (dense->flags & ACM_DENSE_PLANAR) != 0;
	D.mix = (dense->flags & ACM_DENSE_MIX) != 0;
	D.f32 = (opts.flags & ACM_BATCH_PCM_F32) != 0;
	if (nwin && D.row_words > ~0ull / nwin)
		return ACMHIP_ERR_ARG;
	D.out_words = nwin * D.row_words;
	if (opts.d_pcm_words < D.out_words)
		return ACMHIP_ERR_ARG;
	/* a converting row's record carries its mode above the count of its samples, of which it has 2 * frames at most */
	if (D.mix && D.frames > (ACM_DENSE_COUNT_MASK >> 1))
		return ACMHIP_ERR_ARG;
	/* an item that is not ACM, or whose index it cannot have, has no channel count: its windows deliver nothing anyway */
	auto has_chans = [&](const acm_batch_window &w) { return w.item < n && items[w.item].ok; };
	/* ... and with ACM_DENSE_MIX one that has the other of the two counts is converted */
	auto converts = [&](const acm_batch_window &w) {
		if (!D.mix || !has_chans(w))
			return false;
		const uint32_t c = items[w.item].info.channels;
		return c != D.channels && (c == 1 || c == 2);
	};
	/* ... and with ACM_DENSE_RESAMPLE one at another rate than the batch's is filtered, or turned away where the ratio is none the
	 * filter takes.  Only a window that is not turned away for its channel count is asked for its rate */
	enum { SAME, FILTERED, BAD };
	auto rate_kind = [&](const acm_batch_window &w, SpeedFilter *f) {
		if (!D.resample || !has_chans(w) || (items[w.item].info.channels != D.channels && !converts(w)))
			return (int)SAME;
		const uint32_t ri = items[w.item].info.rate;
		if (D.speed) {
			/* ... by its rate times its speed, in either form of the filter */
			*f = acm_speed_filter(ri, D.rate, w.reserved ? w.reserved >> 16 : 1, w.reserved ? w.reserved & 0xFFFF : 1);
			return f->kind == SPEED_NONE ? (int)SAME : f->kind == SPEED_BAD ? (int)BAD : (int)FILTERED;
		}
		if (ri == D.rate)
			return (int)SAME;
		ResampleRatio r;
		if (!acm_resample_ratio(ri, D.rate, &r))
			return (int)BAD;
		*f = SpeedFilter();
		f->kind = SPEED_EXACT;
		f->L = r.L, f->M = r.M, f->K = r.K, f->Wd = r.Wd;
		return (int)FILTERED;
	};
	for (size_t k = 0; k < nwin; k++) {
		/* whole frames, T of them at most - of the batch's channel count, or of the item's own where the window is converted */
		const uint32_t c = converts(wins[k]) ? items[wins[k].item].info.channels : D.channels;
		if (wins[k].max_words > D.frames * c || wins[k].first_word % c || wins[k].max_words % c) {
			/* ... T frames of the batch's rate: a filtered window may be M / L times as long (8 times at most) */
			SpeedFilter r;
			if (wins[k].first_word % c || wins[k].max_words % c || rate_kind(wins[k], &r) != FILTERED)
				return ACMHIP_ERR_ARG;
			if (wins[k].max_words / c > ACM_RESAMPLE_MAX_DOWN * D.frames || acm_resample_frames(wins[k].max_words / c, r.L, r.M) > D.frames)
				return ACMHIP_ERR_ARG;
		} else if (D.resample) {
			SpeedFilter r;
			if (rate_kind(wins[k], &r) == FILTERED && acm_resample_frames(wins[k].max_words / c, r.L, r.M) > D.frames)
				return ACMHIP_ERR_ARG;
		}
	}

	D.wins.assign(wins, wins + nwin);
	D.rejected.assign(nwin, 0);
	D.mode.assign(nwin, D.channels == 2 && D.planar ? ACM_DENSE_MODE_SPLIT : ACM_DENSE_MODE_COPY);
	for (size_t k = 0; k < nwin; k++) {
		const acm_batch_window &w = wins[k];
		if (!has_chans(w) || items[w.item].info.channels == D.channels)
			continue;
		if (converts(w)) {
			D.mode[k] = D.channels == 1 ? ACM_DENSE_MODE_DOWN : D.planar ? ACM_DENSE_MODE_UP_PLANAR : ACM_DENSE_MODE_UP_INTER;
		} else {
			D.rejected[k] = 1;
			D.wins[k].max_words = 0;
		}
	}
	if (D.resample) {
		D.bad_ratio.assign(nwin, 0);
		std::vector<int8_t> ratio(nwin, -1);
		std::vector<uint8_t> chans(nwin, (uint8_t)D.channels);
		std::vector<SpeedFilter> filt(nwin);
		for (size_t k = 0; k < nwin; k++) {
			const acm_batch_window &w = wins[k];
			SpeedFilter r;
			const int kind = rate_kind(w, &r);
			if (kind == BAD) {
				D.bad_ratio[k] = D.rejected[k] = 1;
				D.wins[k].max_words = 0;
			}
			if (kind != FILTERED)
				continue;
			/* a table is a function of (L, M), or of the cutoff alone where it is wide */
			auto serves = [&](const ResampleTable &t) {
				return r.kind == SPEED_WIDE ? t.wide && t.c == r.c : !t.wide && t.r.L == r.L && t.r.M == r.M;
			};
			size_t id = 0;
			while (id < D.tables.size() && !serves(*D.tables[id]))
				id++;
			if (id == D.tables.size()) {
				if (id == ACM_RESAMPLE_MAX_RATIOS)
					return ACMHIP_ERR_ARG;
				D.tables.push_back(acm_speed_table(r));
				D.table_rate.push_back(items[w.item].info.rate);
				if (!D.tables.back())
					return ACMHIP_ERR_ARG;
			}
			ratio[k] = (int8_t)id;
			chans[k] = (uint8_t)items[w.item].info.channels;
			filt[k] = r;
		}
		if (!D.tables.empty()) {
			D.ratio.swap(ratio);
			D.chans.swap(chans);
			D.filt.swap(filt);
		}
	}
	D.inner = opts;
	D.inner.d_pcm = nullptr;
	D.inner.d_pcm_words = 0;
	D.inner.flags &= ~ACM_BATCH_PCM_F32;
	return ACMHIP_OK;
}

void acm_dense_report(const DenseLayout &D, const WindowSlot &s, size_t k, acm_batch_window *w)
{
	w->status = D.rejected[k] ? ACMHIP_ERR_ARG : s.status;
	w->words = s.words;
	w->dev_off = w->slot_off = k * D.row_words;
	w->slot_words = D.row_words;
}

bool acm_dense_rows(const DenseLayout &D, const WindowSlot *slots, const acm_batch_window *final, AcmDenseRow *rows)
{
	bool converts = false;
	for (size_t k = 0; k < D.wins.size(); k++) {
		const uint64_t count = slots[k].active ? std::min(final[k].words, slots[k].words) : 0;
		const uint64_t mode = count && D.mode[k] >= ACM_DENSE_MODE_DOWN ? D.mode[k] : 0;       /* a row of zeros is one in any mode */
		rows[k] = AcmDenseRow{ count ? slots[k].dev_off : 0, count | mode << ACM_DENSE_MODE_SHIFT };
		converts |= mode != 0;
	}
	return converts;
}

/* every table of the call, each from a multiple of 8 taps on, zeros up to the next */
static void copy_taps(const DenseLayout &D, int16_t *taps)
{
	for (size_t id = 0; id < D.tables.size(); id++) {
		int16_t *at = taps + D.tap_at(id);
		std::fill(std::copy(D.tables[id]->q.begin(), D.tables[id]->q.end(), at), at + D.tap_words(id), (int16_t)0);
	}
}

bool acm_dense_resample_rows(const DenseLayout &D, const AcmDenseRow *rows, AcmResampleRow *rs, int16_t *taps)
{
	bool filters = false;
	for (size_t k = 0; k < D.wins.size(); k++) {
		const uint64_t count = rows[k].count & ACM_DENSE_COUNT_MASK;
		rs[k] = AcmResampleRow{};
		if (D.ratio[k] < 0 || !count)
			continue;
		const SpeedFilter &r = D.filt[k];
		const uint64_t f = count / D.chans[k];
		rs[k] = AcmResampleRow{ (uint32_t)D.tap_at(D.ratio[k]), r.L, r.M, r.Wd, acm_resample_frames(f, r.L, r.M), f };
		filters = true;
	}
	copy_taps(D, taps);
	return filters;
}

bool acm_dense_wide_rows(const DenseLayout &D, const AcmDenseRow *rows)
{
	for (size_t k = 0; k < D.filt.size(); k++)
		if (D.filt[k].kind == SPEED_WIDE && (rows[k].count & ACM_DENSE_COUNT_MASK))
			return true;
	return false;
}

void acm_dense_speed_rows(const DenseLayout &D, const AcmDenseRow *rows, AcmSpeedRow *sp, int16_t *taps)
{
	for (size_t k = 0; k < D.wins.size(); k++) {
		const uint64_t count = rows[k].count & ACM_DENSE_COUNT_MASK;
		sp[k] = AcmSpeedRow{};
		if (D.ratio[k] < 0 || !count)
			continue;
		const SpeedFilter &r = D.filt[k];
		const uint64_t f = count / D.chans[k];
		sp[k] = AcmSpeedRow{ (uint32_t)D.tap_at(D.ratio[k]), r.L, r.M, r.Wd, acm_resample_frames(f, r.L, r.M), f,
				     r.kind == SPEED_WIDE ? r.step : 0, r.b, r.kind == SPEED_WIDE };
	}
	copy_taps(D, taps);
}

DenseLaunch acm_dense_tables(const DenseLayout &D, const WindowSlot *slots, const acm_batch_window *final, uint8_t *table)
{
	AcmDenseRow *rows = reinterpret_cast<AcmDenseRow *>(table);
	const bool mixed = acm_dense_rows(D, slots, final, rows);
	if (!D.tables.empty()) {
		void *second = table + D.resample_off();
		int16_t *taps = reinterpret_cast<int16_t *>(table + D.taps_off());
		if (acm_dense_wide_rows(D, rows)) {
			acm_dense_speed_rows(D, rows, static_cast<AcmSpeedRow *>(second), taps);
			return DenseLaunch{ DENSE_SPEED, D.table_bytes() };
		}
		if (acm_dense_resample_rows(D, rows, static_cast<AcmResampleRow *>(second), taps))
			return DenseLaunch{ DENSE_RESAMPLE, D.table_bytes() };
	}
	return DenseLaunch{ mixed ? DENSE_MIXED : DENSE_PLAIN, D.row_table_bytes() };
}

} // namespace acmbatch

extern "C" int acmk_dense_layout_visit(const acm_stage_info *info, const uint64_t *len, const uint8_t *ok, const int32_t *end_status,
				       const uint64_t *whole, const acm_block_mark *const *marks, const uint32_t *blocks, size_t n,
				       const uint64_t *win3, size_t nwin, const acm_batch_opts *opts, const acm_dense_opts *dense,
				       const uint64_t *final_words, acmk_window_layout_visit_fn visit, void *ctx)
{
	return acmk_dense_speed_layout_visit(info, len, ok, end_status, whole, marks, blocks, n, win3, nullptr, nwin, opts, dense, final_words, visit, ctx);
}

extern "C" int acmk_dense_speed_layout_visit(const acm_stage_info *info, const uint64_t *len, const uint8_t *ok, const int32_t *end_status,
					     const uint64_t *whole, const acm_block_mark *const *marks, const uint32_t *blocks, size_t n,
					     const uint64_t *win3, const uint32_t *speeds, size_t nwin, const acm_batch_opts *opts,
					     const acm_dense_opts *dense, const uint64_t *final_words, acmk_window_layout_visit_fn visit, void *ctx)
{
	using namespace acmbatch;
	std::vector<WindowItem> items(n);
	for (size_t i = 0; i < n; i++) {
		items[i].info = info[i];
		items[i].len = len[i];
		items[i].ok = ok[i] != 0;
		items[i].end_status = end_status[i];
		items[i].whole = whole[i];
		items[i].marks = marks[i];
		items[i].blocks = blocks[i];
	}
	std::vector<acm_batch_window> wins(nwin);
	for (size_t k = 0; k < nwin; k++) {
		wins[k] = acm_batch_window{};
		wins[k].item = (uint32_t)win3[3 * k];
		wins[k].reserved = speeds ? speeds[k] : 0;
		wins[k].first_word = win3[3 * k + 1];
		wins[k].max_words = win3[3 * k + 2];
	}
	DenseLayout D;
	WindowLayout L;
	int rc = acm_dense_prepare(items.data(), n, wins.data(), nwin, *opts, dense, &D);
	if (rc == ACMHIP_OK)
		rc = acm_window_layout(items.data(), n, D.wins.data(), nwin, D.inner, &L);
	if (rc == ACMHIP_OK) {
		std::vector<uint64_t> w, rej(D.rejected.begin(), D.rejected.end()), rep;
		for (size_t k = 0; k < nwin; k++) {
			w.insert(w.end(), { (uint64_t)D.wins[k].item, D.wins[k].first_word, D.wins[k].max_words });
			acm_dense_report(D, L.slots[k], k, &wins[k]);
			rep.insert(rep.end(), { (uint64_t)(int64_t)wins[k].status, wins[k].words, wins[k].dev_off, wins[k].slot_off, wins[k].slot_words });
			if (final_words)
				wins[k].words = final_words[k];
		}
		/* the tables as the driver fills them, and the kernel it launches */
		std::vector<uint8_t> table(D.table_bytes());
		const DenseLaunch launch = acm_dense_tables(D, L.slots.data(), wins.data(), table.data());
		const AcmDenseRow *rows = reinterpret_cast<const AcmDenseRow *>(table.data());
		/* row k's record of the second table, where the launch reads one: an AcmResampleRow is the head of an AcmSpeedRow that is not wide */
		auto second = [&](size_t k) {
			AcmSpeedRow r{};
			const uint8_t *at = table.data() + D.resample_off();
			if (launch.kernel == DENSE_SPEED)
				memcpy(&r, at + k * sizeof(AcmSpeedRow), sizeof(AcmSpeedRow));
			else if (launch.kernel == DENSE_RESAMPLE)
				memcpy(&r, at + k * sizeof(AcmResampleRow), sizeof(AcmResampleRow));
			return r;
		};
		/* ... and its frames where it is not filtered */
		auto frames_of = [&](size_t k) {
			const uint32_t c = (rows[k].count >> ACM_DENSE_MODE_SHIFT) ? 3 - D.channels : D.channels;
			return (rows[k].count & ACM_DENSE_COUNT_MASK) / c;
		};
		if (nwin) {
			visit(ctx, "wins", w.data(), 3 * sizeof(uint64_t), nwin);
			visit(ctx, "rejected", rej.data(), sizeof(uint64_t), nwin);
			visit(ctx, "report", rep.data(), 5 * sizeof(uint64_t), nwin);
			visit(ctx, "rows", rows, sizeof(AcmDenseRow), nwin);
		}
		if (D.mix) {
			std::vector<uint64_t> mix(D.mode.begin(), D.mode.end());
			bool converts = false;
			for (size_t k = 0; k < nwin; k++)
				converts |= (rows[k].count >> ACM_DENSE_MODE_SHIFT) != 0;
			mix.push_back(converts);
			visit(ctx, "mix", mix.data(), sizeof(uint64_t), mix.size());
		}
		if (D.speed) {
			std::vector<uint64_t> res, tabs;
			for (size_t k = 0; k < nwin; k++) {
				const AcmSpeedRow r = second(k);
				if (r.L)
					res.insert(res.end(), { r.wide ? 2ull : 1ull, (uint64_t)r.L, (uint64_t)r.M, (uint64_t)D.ratio[k], r.n_out, r.step, (uint64_t)r.b,
								(uint64_t)r.Wd });
				else
					res.insert(res.end(), { D.bad_ratio[k] ? ~0ull : 0ull, (uint64_t)!D.bad_ratio[k], (uint64_t)!D.bad_ratio[k], ~0ull, frames_of(k), 0, 0, 0 });
			}
			res.insert(res.end(), { launch.kernel == DENSE_SPEED ? 2ull : launch.kernel == DENSE_RESAMPLE ? 1ull : 0ull, 0, 0, 0, 0, 0, 0, 0 });
			for (size_t id = 0; id < D.tables.size(); id++) {
				const ResampleTable &t = *D.tables[id];
				tabs.insert(tabs.end(), { (uint64_t)t.wide, (uint64_t)t.c, (uint64_t)t.r.L, (uint64_t)t.r.M, (uint64_t)t.r.K, (uint64_t)t.r.Wd,
							  (uint64_t)t.phases(), (uint64_t)D.tap_at(id) });
			}
			visit(ctx, "speed", res.data(), 8 * sizeof(uint64_t), nwin + 1);
			visit(ctx, "speed_tables", tabs.data(), 8 * sizeof(uint64_t), D.tables.size());
		} else if (D.resample) {
			std::vector<uint64_t> res, tabs;
			for (size_t k = 0; k < nwin; k++) {
				const AcmSpeedRow r = second(k);
				if (r.L)
					res.insert(res.end(), { (uint64_t)r.L, (uint64_t)r.M, (uint64_t)D.ratio[k], r.n_out, 0 });
				else
					res.insert(res.end(), { (uint64_t)!D.bad_ratio[k], (uint64_t)!D.bad_ratio[k], ~0ull, frames_of(k), (uint64_t)D.bad_ratio[k] });
			}
			res.insert(res.end(), { (uint64_t)(launch.kernel == DENSE_RESAMPLE), 0, 0, 0, 0 });
			for (size_t id = 0; id < D.tables.size(); id++) {
				const ResampleTable &t = *D.tables[id];
				tabs.insert(tabs.end(), { (uint64_t)D.table_rate[id], (uint64_t)t.r.L, (uint64_t)t.r.M, (uint64_t)t.r.K, (uint64_t)t.r.Wd, (uint64_t)D.tap_at(id) });
			}
			visit(ctx, "resample", res.data(), 5 * sizeof(uint64_t), nwin + 1);
			visit(ctx, "tables", tabs.data(), 6 * sizeof(uint64_t), D.tables.size());
		}
	}
	const uint64_t totals[] = { D.frames, D.row_words, D.channels, (uint64_t)D.planar, (uint64_t)D.f32, D.out_words, D.pcm_arena_words(L.pcm_total),
				    L.blocks_parsed, D.table_off(L), D.table_bytes(), (uint64_t)(int64_t)rc };
	visit(ctx, "totals", totals, sizeof(uint64_t), sizeof(totals) / sizeof(totals[0]));
	return rc;
}
