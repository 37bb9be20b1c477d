/*
 * acm_batch_layout.cpp - the device-free half of the batch front end (acm_batch.cpp): arena layout, chunks, parse groups, the device
 * parser's jobs, block ranges and stripes, and every decision about the way the batch travels.  Plain C++; see acm_batch_layout.h.
 */
#include "acm_batch_layout.h"

#include <stdlib.h>

namespace acmbatch {

bool lean_form_level(uint32_t level)
{
	const int T2 = acmk_tile2_rows(level), TM = acmk_tile2m_rows(level);
	return acmk_tile2m_stages(level) == 6 && T2 > 0 && TM > 0 && T2 % TM == 0 && level <= ACM_K1_MAX_LEVEL;
}

namespace {

/* an integer switch of the tuning build's environment (ACM_TUNING_ENV), `unset` in the product */
int tuning_switch(const char *value, int unset) { return value ? atoi(value) : unset; }

/* chunks of whole streams: about 1/16 of the batch each, but not below 8 MiB of staged indices */
void cut_chunks(const LayoutItem *items, size_t n, BatchLayout &L)
{
	const uint64_t chunk_target = std::max<uint64_t>(4u << 20, L.idx_total / 16);
	std::vector<size_t> starts{ 0 };
	uint64_t cut_at = 0;
	for (size_t i = 0; i < n; i++)
		if (items[i].ok && L.slots[i].idx_off - cut_at >= chunk_target) {
			starts.push_back(i);
			cut_at = L.slots[i].idx_off;
		}
	L.chunks.resize(starts.size());
	for (size_t c = 0; c < L.chunks.size(); c++) {
		ChunkLayout &ch = L.chunks[c];
		ch.first = starts[c];
		ch.last = (c + 1 < L.chunks.size()) ? starts[c + 1] : n;
		bool any = false;
		for (size_t i = ch.first; i < ch.last; i++) {
			SlotLayout &s = L.slots[i];
			if (!items[i].ok)
				continue;
			s.chunk = (uint32_t)c;
			if (!any) {
				ch.idx_begin = s.idx_off;
				ch.hdr_begin = s.hdr_off;
				any = true;
			}
			ch.idx_end = s.idx_off + s.idx_len;
			ch.hdr_end = s.hdr_off + s.need_blocks;
		}
	}
}

/* the packed staged form (opt-in, host parsing): chunk-table entries are reserved per stream from what the headers promise;
 * a pipeline chunk's blobs share the region of the blob arena that mirrors its slice of the int16 arena (a stream whose
 * packed form does not fit there - indices that need 16 bits throughout - simply travels as int16) */
void reserve_packed(const LayoutItem *items, BatchLayout &L)
{
	for (ChunkLayout &ch : L.chunks) {
		ch.pk_chunk_begin = L.pk_chunks_total;
		for (size_t i = ch.first; i < ch.last; i++) {
			SlotLayout &s = L.slots[i];
			const acm_stage_info &f = items[i].info;
			const int tr = items[i].ok ? acmhip_packed_tile_rows(f.level) : 0;
			if (tr <= 0)
				continue;
			s.pk_chunk_off = L.pk_chunks_total;
			s.pk_chunk_cap = s.need_blocks * f.rows / (uint64_t)tr * (uint64_t)acmhip_packed_slots(f.level);
			L.pk_chunks_total += s.pk_chunk_cap;
		}
		ch.pk_chunk_end = L.pk_chunks_total;
	}
}

/* the byte-plane staged form (the default; ACM_BATCH_STAGE_INT16 turns it off): every stream of a level the matrix-core build covers
 * gets room for its rows plus the two rows of zeros in front */
void reserve_mform(const LayoutItem *items, BatchLayout &L)
{
	for (ChunkLayout &ch : L.chunks) {
		ch.mf_begin = L.mf_total;
		ch.mf_pair_begin = L.mf_pairs_total;
		for (size_t i = ch.first; i < ch.last; i++) {
			SlotLayout &s = L.slots[i];
			const acm_stage_info &f = items[i].info;
			if (!items[i].ok || acmhip_mform_tile_rows(f.level) <= 0)
				continue;
			s.mf_off = L.mf_total;
			s.mf_rows_cap = (s.need_blocks * f.rows) & ~1ull;
			s.mf_pair_off = L.mf_pairs_total;
			L.mf_total += (acmhip_mform_bytes(f.level, s.mf_rows_cap) + 255) & ~255ull;
			L.mf_pairs_total += acmhip_mform_pairs(s.mf_rows_cap);
		}
		ch.mf_end = L.mf_total;
		ch.mf_pair_end = L.mf_pairs_total;
	}
}

/* AUTO: the device walk takes as long as the longest stream takes one wavefront, the host pool takes total / threads.
 * Measured (profiles/r2_parse_probe.txt): a wavefront alone on its SIMD walks at ~1/5 of a host core's parsing rate
 * (up to 1024 streams), with four per SIMD at ~1/9 (up to the 32 K streams acm_parse_scan_wave takes), a lane of
 * acm_parse_scan at ~1/16: device when the batch is worth more than that many x threads streams of the longest one */
bool auto_dev_parse(const LayoutItem *items, size_t n, const BatchLayout &L, int threads_wanted)
{
	uint64_t longest = 0;
	for (size_t i = 0; i < n; i++)
		if (items[i].ok)
			longest = std::max(longest, L.slots[i].idx_len);
	const uint64_t per_thread = n <= 1024 ? 5 : n <= 32768 ? 9 : 16;
	return longest > 0 && L.idx_total / longest >= per_thread * (uint64_t)threads_wanted;
}

/* Block ranges (device parsing of a big batch into host buffers): the walk of a stream is one wavefront's sequential job -
 * 33 ms for two megasamples - and nothing can be synthesised or read back before it ends.  So the walk is cut into R
 * launches, each taking every stream R-th of its blocks further (the bit offset it stopped at stays on the device), and
 * the synthesis and the read-back of range r run while range r + 1 is walked.  The PCM arenas are range-major for that:
 * range r of every stream back to back, one transfer per range; the copy-out puts the pieces where the caller wants them. */
size_t range_count(const acm_batch_opts &opts, const BatchLayout &L, size_t ok_streams)
{
	/* a range of ~128 Msamples is walked in ~2 ms and read back in ~5: 2 ... 16 ranges from 256 Msamples on (measured on
	 * the 2.1-Gsample batch: 0.136 / 0.114 / 0.106 / 0.104 s with 1 / 4 / 8 / 16 ranges, profiles/r3_batch_timeline.txt) */
	size_t want = L.idx_total >= (256u << 20) ? (size_t)std::min<uint64_t>(16, L.idx_total >> 27) : 1;
	if ((opts.flags >> 8) & 0xFFu)                          /* ACM_BATCH_RANGES(n): the caller's count (1 = in one piece) */
		want = (opts.flags >> 8) & 0xFFu;
	else if (ACM_TUNING_ENV("ACM_BATCH_RANGES"))
		want = (size_t)std::max(1, tuning_switch(ACM_TUNING_ENV("ACM_BATCH_RANGES"), 1));
	if (want > 1 && want <= 64 && L.dev_parse && !L.keep_on_device && !L.dev_ids.empty() && L.dev_ids.size() == ok_streams &&
	    L.dev_ids.size() <= ACM_PARSE_RANGE_MAX_STREAMS)
		return want;
	return 1;
}

/* the range-major PCM arenas of R > 1 ranges */
void cut_ranges(const LayoutItem *items, size_t n, BatchLayout &L)
{
	const size_t R = L.R;
	/* where a stream may travel in the byte-plane form a range has to end on a whole tile of the lean kernel (the plan of a range is a
	 * window; its ragged end would need int16 rows nobody writes) - which also keeps the row pairs of an odd block height, every
	 * other one of which lies across two blocks, inside one range.  Blocks that are whole tiles: unit 1, ranges as ever */
	for (size_t i = 0; i < n; i++) {
		if (!items[i].ok || !lean_form_level(items[i].info.level))
			continue;
		const uint32_t T2 = (uint32_t)acmk_tile2_rows(items[i].info.level);
		uint32_t a = items[i].info.rows, b = T2;
		while (b) {
			const uint32_t t = a % b;
			a = b;
			b = t;
		}
		L.slots[i].range_unit = T2 / a;
	}
	L.piece_off.assign(R * n, 0);
	L.piece_len.assign(R * n, 0);
	L.rbase.assign(R + 1, 0);
	uint64_t at = 0;
	for (size_t r = 0; r < R; r++) {
		L.rbase[r] = at;
		for (size_t i = 0; i < n; i++) {
			const SlotLayout &s = L.slots[i];
			const acm_stage_info &f = items[i].info;
			if (!items[i].ok)
				continue;
			const uint64_t bl = (uint64_t)f.rows * f.cols;
			const uint64_t words = deliverable_words(f.total_values, bl, f.channels, s.need_blocks);
			const uint64_t lo = std::min(words, (uint64_t)acmk_range_bound((uint32_t)s.need_blocks, (uint32_t)r, (uint32_t)R, s.range_unit) * bl);
			const uint64_t hi = std::min(words, (uint64_t)acmk_range_bound((uint32_t)s.need_blocks, (uint32_t)r + 1u, (uint32_t)R, s.range_unit) * bl);
			L.piece_off[r * n + i] = at;
			L.piece_len[r * n + i] = hi - lo;
			at += round_up(hi - lo, 64);
		}
	}
	L.rbase[R] = at;
	L.pcm_arena_words = std::max(at, L.pcm_total);
}

/* 2a. device parsing: the job of every stream the device parser takes, and the files of one chunk as an upload piece */
void build_jobs(const LayoutItem *items, BatchLayout &L)
{
	const size_t nd = L.dev_ids.size();
	L.groups.resize(L.chunks.size());
	L.jobs.resize(nd);
	uint64_t col_off = 0;
	for (GroupLayout &g : L.groups)
		g.k_first = g.k_last = nd;
	for (size_t k = 0; k < nd; k++) {
		const size_t i = L.dev_ids[k];
		SlotLayout &s = L.slots[i];
		const acm_stage_info &f = items[i].info;
		s.on_dev = true;
		AcmParseJob &j = L.jobs[k];
		j.file_off = s.file_off;
		j.idx_off = s.idx_off;
		j.hdr_off = s.hdr_off;
		j.col_off = col_off;
		j.file_len = (uint32_t)items[i].len;
		j.data_start = (uint32_t)f.header_bytes;
		j.level = f.level;
		j.rows = f.rows;
		j.blocks = (uint32_t)s.need_blocks;
		j.range_unit = s.range_unit;
		j.mf_off = j.mf_pair_off = j.mf_rows = 0;
		if (L.dev_mform && s.mf_rows_cap && lean_form_level(f.level)) {
			/* rows [0, mf_rows) - the whole tiles of the lean kernel, as the plan will cut them - are staged in the byte-plane form.
			 * With block ranges every range ends on a tile boundary (SlotLayout::range_unit, above) */
			const uint64_t T2 = (uint64_t)acmk_tile2_rows(f.level), TM = (uint64_t)acmk_tile2m_rows(f.level);
			const uint64_t words = deliverable_words(f.total_values, (uint64_t)f.rows * f.cols, f.channels, s.need_blocks);
			const uint64_t rows2 = std::min<uint64_t>(s.need_blocks * f.rows, words >> f.level) / T2 * T2;
			if (rows2 && rows2 <= s.mf_rows_cap && rows2 < (1ull << 32)) {
				j.mf_off = s.mf_off;
				j.mf_pair_off = (uint32_t)s.mf_pair_off;
				j.mf_rows = (uint32_t)rows2;
				s.pk_ntiles = (uint32_t)(rows2 / TM);
			}
		}
		col_off += s.need_blocks << f.level;
		GroupLayout &g = L.groups[s.chunk];
		if (g.k_first == nd) {
			g.k_first = k;
			g.file_begin = s.file_off;
		}
		g.k_last = k + 1;
		g.file_end = s.file_off + file_slot_bytes(items[i].len);
		g.max_columns = std::max<uint64_t>(g.max_columns, s.need_blocks << f.level);
	}
}

/* block ranges: the files go up in R stripes (stripe s of every file back to back: one transfer, then a scatter kernel),
 * so that range 0 is walked, synthesised and on its way back while the later stripes are still going up */
void cut_stripes(const LayoutItem *items, BatchLayout &L)
{
	const size_t R = L.R, nd = L.dev_ids.size();
	L.stripe_at.assign(R * nd, 0);
	L.stripe_base.assign(R + 1, 0);
	uint64_t at = 0;
	for (size_t s = 0; s < R; s++) {
		L.stripe_base[s] = at;
		for (size_t k = 0; k < nd; k++) {
			const uint32_t len = (uint32_t)items[L.dev_ids[k]].len;
			L.stripe_at[s * nd + k] = at;
			at += acmk_stripe_bound(len, (uint32_t)s + 1, (uint32_t)R) - acmk_stripe_bound(len, (uint32_t)s, (uint32_t)R);
		}
	}
	L.stripe_base[R] = at;          /* == files_total: the stripes tile every slot */
}

} // namespace

int acm_batch_layout(const LayoutItem *items, size_t n, const acm_batch_opts &opts, int threads_wanted, bool prestaged, BatchLayout *out)
{
	BatchLayout &L = *out;
	L = BatchLayout{};
	/* 1. headers -> arena layout */
	L.slots.resize(n);
	Int16Arenas arenas;
	size_t ok_streams = 0;
	for (size_t i = 0; i < n; i++) {
		SlotLayout &s = L.slots[i];
		if (!items[i].ok)
			continue;
		s.idx_len = arenas.place(items[i].info, items[i].len, &s.need_blocks, &s.idx_off, &s.hdr_off);
		s.pcm_off = s.idx_off;
		ok_streams++;
	}
	L.idx_total = L.pcm_total = L.pcm_arena_words = arenas.idx_total;
	L.hdr_total = arenas.hdr_total;
	L.keep_on_device = opts.d_pcm != nullptr;
	/* pinned caller buffers: the copy engine writes every stream's PCM where the caller wants it (one transfer per
	 * stream, so only for streams big enough that the per-transfer cost disappears) */
	L.direct_out = !L.keep_on_device && (opts.flags & ACM_BATCH_PCM_PINNED) && n > 0 && L.pcm_total / n >= 32768;
	if (L.keep_on_device && opts.d_pcm_words < L.pcm_total)
		return ACMHIP_ERR_ARG;
	cut_chunks(items, n, L);

	/* (no second form where the plans may not use the lean kernels that read it) */
	const bool lean_off = (opts.plan_flags & ACMHIP_PLAN_NO_LEAN) || tuning_switch(ACM_TUNING_ENV("ACM_K2"), 1) == 0;
	const bool second_form = !lean_off && !(opts.plan_flags & ACMHIP_PLAN_STAGEWISE);
	L.stage_packed = (opts.flags & ACM_BATCH_STAGE_PACKED) && second_form;
	if (L.stage_packed)
		reserve_packed(items, L);
	/* (blocks parsed ahead of time are int16 rows already: re-ordering them is a pass of its own, taken only when asked for) */
	const bool mform_default = !(opts.flags & (ACM_BATCH_STAGE_INT16 | ACM_BATCH_STAGE_PACKED)) && !prestaged;
	L.stage_mform = ((opts.flags & ACM_BATCH_STAGE_BYTEPLANE) || mform_default) && second_form;
	if (L.stage_mform) {
		L.stage_packed = false;         /* one second form per batch */
		reserve_mform(items, L);
	}

	/* (blocks parsed ahead of time: the host pool only moves them into the upload arenas) */
	L.dev_parse = !prestaged && (opts.parse == ACM_BATCH_PARSE_DEVICE || (opts.parse == ACM_BATCH_PARSE_AUTO && auto_dev_parse(items, n, L, threads_wanted)));
	/* the device parser writes the byte-plane form itself where a stream can have it (the chunk kernel's levels, even acm_rows): rows the
	 * lean kernels take never exist as int16 then (acm_parse.hip: acm_parse_columns); the host pool's second forms are host-parsing only */
	if (L.dev_parse) {
		L.dev_mform = L.stage_mform && tuning_switch(ACM_TUNING_ENV("ACM_BATCH_DEV_MFORM"), 1) != 0;
		L.stage_packed = L.stage_mform = false;
		for (size_t i = 0; i < n; i++) {
			SlotLayout &s = L.slots[i];
			if (!items[i].ok || !acmk_parse_supported(items[i].info.level, items[i].info.rows, items[i].len, s.need_blocks))
				continue;
			s.file_off = L.files_total;
			L.files_total += file_slot_bytes(items[i].len);
			L.cols_total += s.need_blocks << items[i].info.level;
			L.dev_ids.push_back(i);
		}
	}
	L.R = range_count(opts, L, ok_streams);
	if (L.R > 1) {
		L.direct_out = false;   /* one transfer per range into the library's arena; pinned caller buffers make the copy-out fault-free */
		cut_ranges(items, n, L);
	}

	/* a second form nobody would stage, or one the tables cannot address (the pair table counts 64-byte units in 30 bits; the device
	 * parser's kernel for it takes ACM_PARSE_RANGE_MAX_STREAMS streams): the batch travels as int16 */
	const bool mf_fits = L.mf_total && (L.mf_total >> 6) < (1ull << 30);
	L.stage_packed = L.stage_packed && L.pk_chunks_total;
	L.stage_mform = L.stage_mform && mf_fits;
	L.dev_mform = L.dev_mform && mf_fits && L.dev_ids.size() <= ACM_PARSE_RANGE_MAX_STREAMS;

	const size_t nd = L.dev_ids.size();
	L.jobs_bytes = round_up(nd * sizeof(AcmParseJob), 64);
	L.res_bytes = nd * (sizeof(AcmParseResult) + sizeof(uint32_t));        /* results, then flags */
	L.stripe_tab_off = L.jobs_bytes + round_up(L.res_bytes, 64);
	L.stripe_tab_bytes = L.R > 1 ? L.R * nd * sizeof(uint64_t) : 0;
	if (nd)
		build_jobs(items, L);
	if (L.R > 1)
		cut_stripes(items, L);
	for (size_t i = 0; i < n; i++) {
		if (items[i].ok && !L.slots[i].on_dev)
			L.host_ids.push_back(i);
		/* the pool hands finished PCM out to the callers' buffers unless it stays on the device or the copy engine delivers it */
		if (items[i].ok && items[i].has_pcm && !L.keep_on_device && !L.direct_out)
			L.out_ids.push_back(i);
	}
	return ACMHIP_OK;
}

} // namespace acmbatch

extern "C" int acmk_batch_layout_visit(const acm_stage_info *info, const uint64_t *len, const uint8_t *ok, const uint8_t *has_pcm, size_t n,
				       const acm_batch_opts *opts, int threads_wanted, int prestaged, acmk_layout_visit visit, void *ctx)
{
	using namespace acmbatch;
	std::vector<LayoutItem> items(n);
	for (size_t i = 0; i < n; i++) {
		items[i].info = info[i];
		items[i].len = len[i];
		items[i].ok = ok[i] != 0;
		items[i].has_pcm = has_pcm[i] != 0;
	}
	BatchLayout L;
	const int rc = acm_batch_layout(items.data(), n, *opts, threads_wanted, prestaged != 0, &L);
	if (rc != ACMHIP_OK)
		return rc;
	std::vector<uint64_t> w;
	auto show = [&](const char *name, size_t per) {
		if (!w.empty())
			visit(ctx, name, w.data(), per * sizeof(uint64_t), w.size() / per);
		w.clear();
	};
	for (size_t i = 0; i < n; i++) {
		const SlotLayout &s = L.slots[i];
		w.insert(w.end(), { s.need_blocks, s.idx_off, s.hdr_off, s.pcm_off, s.idx_len, s.chunk, s.pk_chunk_off, s.pk_chunk_cap, s.pk_ntiles,
				    s.mf_off, s.mf_rows_cap, s.mf_pair_off, s.range_unit, s.file_off, s.on_dev, items[i].ok });
	}
	show("slots", 16);
	for (const ChunkLayout &c : L.chunks)
		w.insert(w.end(), { c.first, c.last, c.idx_begin, c.idx_end, c.hdr_begin, c.hdr_end, c.pk_chunk_begin, c.pk_chunk_end, c.mf_begin,
				    c.mf_end, c.mf_pair_begin, c.mf_pair_end });
	show("chunks", 12);
	for (const GroupLayout &g : L.groups)
		w.insert(w.end(), { g.k_first, g.k_last, g.file_begin, g.file_end, g.max_columns });
	show("groups", 5);
	const std::pair<const char *, const std::vector<size_t> *> ids[] = { { "dev_ids", &L.dev_ids }, { "host_ids", &L.host_ids }, { "out_ids", &L.out_ids } };
	for (const auto &t : ids) {
		w.assign(t.second->begin(), t.second->end());
		show(t.first, 1);
	}
	if (!L.jobs.empty())
		visit(ctx, "jobs", L.jobs.data(), sizeof(AcmParseJob), L.jobs.size());
	const std::pair<const char *, const std::vector<uint64_t> *> tabs[] = { { "piece_off", &L.piece_off }, { "piece_len", &L.piece_len }, { "rbase", &L.rbase },
										 { "stripe_at", &L.stripe_at }, { "stripe_base", &L.stripe_base } };
	for (const auto &t : tabs) {
		w = *t.second;
		show(t.first, 1);
	}
	w = { L.idx_total, L.hdr_total, L.pcm_total, L.pcm_arena_words, L.pk_chunks_total, L.mf_total, L.mf_pairs_total, L.files_total, L.cols_total,
	      L.jobs_bytes, L.res_bytes, L.stripe_tab_off, L.stripe_tab_bytes, L.R, L.stage_packed, L.stage_mform, L.dev_parse, L.dev_mform,
	      L.direct_out, L.keep_on_device, (uint64_t)rc };
	visit(ctx, "totals", w.data(), sizeof(uint64_t), w.size());
	return rc;
}
