/*
 * acm_window_layout.cpp - the device-free half of the windowed batch decode (acm_batch_windows.cpp): which blocks a window needs,
 * where its rows, headers, columns, file span and PCM slot sit, which windows the device parser may take, the records it reads
 * and the size of the job arena.  No HIP call here.
 */
#include "acm_window_layout.h"

#include "acm_pool.h"

namespace acmbatch {

int acm_window_layout(const WindowItem *items, size_t n, const acm_batch_window *wins, size_t nwin, const acm_batch_opts &opts, WindowLayout *out,
		      Pool *pool)
{
	WindowLayout &L = *out;
	L = WindowLayout();
	L.slots.resize(nwin);
	/* the windows: block ranges and the int16 arenas */
	for (size_t k = 0; k < nwin; k++) {
		const acm_batch_window &w = wins[k];
		WindowSlot &s = L.slots[k];
		s.dev_off = s.slot_off = L.pcm_total;
		if (w.item >= n) {
			s.status = ACMHIP_ERR_ARG;
			continue;
		}
		const WindowItem &it = items[w.item];
		const uint64_t words = window_words(it.whole, w.first_word, w.max_words);
		s.status = words == w.max_words ? ACM_OK : it.end_status;
		if (!words)
			continue;
		const uint64_t cols = it.info.cols, rows = it.info.rows;
		const uint64_t first_row = w.first_word / cols, last_row = (w.first_word + words - 1) / cols;
		s.b0 = (uint32_t)((first_row > 2 ? first_row - 2 : 0) / rows);
		s.nb = (uint32_t)(last_row / rows + 1 - s.b0);
		s.row_begin = (uint32_t)(first_row - (uint64_t)s.b0 * rows);
		s.lead = w.first_word - first_row * cols;
		s.active = true;
		s.idx_off = L.idx_total;
		s.hdr_off = L.hdr_total;
		s.words = words;
		s.slot_words = window_slot_words(s.lead, words);
		s.dev_off = s.slot_off + s.lead;
		L.idx_total += round_up(window_rows_words(it.info, s.nb), 64);
		L.hdr_total += s.nb;
		L.pcm_total += s.slot_words;
		L.blocks_parsed += s.nb;
		L.act.push_back(k);
	}
	L.dev_parse = opts.parse == ACM_BATCH_PARSE_DEVICE || (opts.parse == ACM_BATCH_PARSE_AUTO && L.blocks_parsed >= ACM_WINDOWS_AUTO_BLOCKS);
	/* who parses: the device takes the windows whose byte span its 32-bit arithmetic covers and whose marks lie inside the span */
	for (size_t k : L.act) {
		WindowSlot &s = L.slots[k];
		const WindowItem &it = items[wins[k].item];
		if (L.dev_parse) {
			/* the bytes that hold the window's blocks, from a dword boundary of the file; offsets inside count from there */
			const acm_block_mark *mk = it.marks;
			s.span_lo = (mk[s.b0].bit >> 3) & ~3ull;
			const uint64_t end_bit = mk[s.b0 + s.nb].bit - 8 * s.span_lo;
			s.span_len = std::min<uint64_t>(it.len, (mk[s.b0 + s.nb].bit + 7) >> 3) - s.span_lo;
			s.on_device = acmk_parse_supported(it.info.level, it.info.rows, s.span_len, s.nb) && end_bit <= 8 * s.span_len;
		}
		if (!s.on_device) {
			L.host_ids.push_back(k);
			continue;
		}
		s.file_off = L.files_total;
		s.col_off = L.cols_total;
		L.files_total += file_slot_bytes(s.span_len);
		L.cols_total += (uint64_t)s.nb * it.info.cols;
		L.max_columns = std::max(L.max_columns, (uint64_t)s.nb * it.info.cols);
		L.dev_ids.push_back(k);
	}
	if (opts.d_pcm && opts.d_pcm_words < L.pcm_total)
		return ACMHIP_ERR_ARG;
	if (L.dev_ids.size() > 0xFFFFFFFFull || L.hdr_total > 0xFFFFFFFFull)
		return ACMHIP_ERR_ARG;

	/* the device parser's records: a job per window, a walk per block checked against its marks */
	const size_t nd = L.dev_ids.size();
	std::vector<uint64_t> bj_at(nd + 1, 0);         /* where every job's block jobs begin */
	for (size_t a = 0; a < nd; a++)
		bj_at[a + 1] = bj_at[a] + L.slots[L.dev_ids[a]].nb;
	L.jobs.resize(nd);
	L.bjobs.resize(bj_at[nd]);
	auto fill = [&](size_t a) {
		const size_t k = L.dev_ids[a];
		const WindowSlot &s = L.slots[k];
		const WindowItem &it = items[wins[k].item];
		const acm_block_mark *mk = it.marks + s.b0;
		AcmParseJob j{};
		j.file_off = s.file_off;
		j.idx_off = s.idx_off;
		j.hdr_off = s.hdr_off;
		j.col_off = s.col_off;
		j.file_len = (uint32_t)s.span_len;      /* a walk can never leave its span */
		j.level = it.info.level;
		j.rows = it.info.rows;
		j.blocks = s.nb;
		j.range_unit = 1;
		L.jobs[a] = j;
		for (uint32_t b = 0; b < s.nb; b++)
			L.bjobs[bj_at[a] + b] = AcmBlockJob{ (uint32_t)a, b, (uint32_t)(mk[b].bit - 8 * s.span_lo), (uint32_t)(mk[b + 1].bit - 8 * s.span_lo),
							     mk[b].val << 4 | mk[b].pwr, 0 };
	};
	if (pool)
		pool->run(nd, fill);
	else
		for (size_t a = 0; a < nd; a++)
			fill(a);
	L.jobs_bytes = round_up(L.jobs.size() * sizeof(AcmParseJob), 64);
	L.bjobs_bytes = round_up(L.bjobs.size() * sizeof(AcmBlockJob), 64);
	L.res_bytes = L.jobs.size() * (sizeof(AcmParseResult) + sizeof(uint32_t));      /* results, then flags */
	return ACMHIP_OK;
}

} // namespace acmbatch

extern "C" int acmk_window_layout_visit(const acm_stage_info *info, const uint64_t *len, const uint8_t *ok, const int32_t *end_status,
					const uint64_t *whole, const acm_block_mark *const *marks, const uint32_t *blocks, size_t n,
					const uint64_t *win3, size_t nwin, const acm_batch_opts *opts, acmk_window_layout_visit_fn visit, void *ctx)
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
		wins[k].first_word = win3[3 * k + 1];
		wins[k].max_words = win3[3 * k + 2];
	}
	WindowLayout L;
	const int rc = acm_window_layout(items.data(), n, wins.data(), nwin, *opts, &L);
	std::vector<uint64_t> w;
	for (const WindowSlot &s : L.slots)
		w.insert(w.end(), { (uint64_t)(int64_t)s.status, s.words, s.slot_off, s.slot_words, s.dev_off, (uint64_t)s.active, (uint64_t)s.on_device,
				    s.b0, s.nb, s.row_begin, s.lead, s.idx_off, s.hdr_off, s.col_off, s.span_lo, s.span_len, s.file_off });
	if (!w.empty())
		visit(ctx, "slots", w.data(), 17 * sizeof(uint64_t), L.slots.size());
	auto ids = [&](const char *name, const std::vector<size_t> &v) {
		std::vector<uint64_t> u(v.begin(), v.end());
		if (!u.empty())
			visit(ctx, name, u.data(), sizeof(uint64_t), u.size());
	};
	ids("act", L.act);
	ids("dev_ids", L.dev_ids);
	ids("host_ids", L.host_ids);
	if (!L.jobs.empty())
		visit(ctx, "jobs", L.jobs.data(), sizeof(AcmParseJob), L.jobs.size());
	if (!L.bjobs.empty())
		visit(ctx, "bjobs", L.bjobs.data(), sizeof(AcmBlockJob), L.bjobs.size());
	const uint64_t totals[] = { L.idx_total, L.hdr_total, L.pcm_total, L.cols_total, L.files_total, L.max_columns, L.blocks_parsed,
				    L.jobs_bytes, L.bjobs_bytes, L.res_bytes, (uint64_t)L.dev_parse, (uint64_t)(int64_t)rc };
	visit(ctx, "totals", totals, sizeof(uint64_t), sizeof(totals) / sizeof(totals[0]));
	return rc;
}
