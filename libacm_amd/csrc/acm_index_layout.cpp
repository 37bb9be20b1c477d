/*
 * acm_index_layout.cpp - the device-free half of the batch index build (acm_batch_index.cpp): which items the device walks, how
 * many blocks each may leave, where its file image and its marks sit, and how the batch is cut into groups.  No HIP call here.
 */
#include "acm_index_layout.h"

namespace acmbatch {

void acm_index_layout(const IndexItem *items, size_t n, uint64_t budget, IndexLayout *out)
{
	IndexLayout &L = *out;
	L = IndexLayout();
	L.slots.resize(n);
	if (budget == 0)
		budget = ACM_INDEX_GROUP_BYTES;
	IndexGroup g;
	auto close_group = [&]() {
		if (g.k_last == g.k_first)
			return;
		L.half_file_bytes = std::max(L.half_file_bytes, g.file_bytes);
		L.half_marks = std::max(L.half_marks, g.marks);
		L.half_jobs = std::max(L.half_jobs, g.k_last - g.k_first);
		L.groups.push_back(g);
		g = IndexGroup();
		g.k_first = g.k_last = L.dev_ids.size();
	};
	for (size_t i = 0; i < n; i++) {
		const IndexItem &it = items[i];
		IndexSlot &s = L.slots[i];
		bool can_hold = false;
		if (it.ok) {
			const uint64_t bl = (uint64_t)it.info.rows * it.info.cols;
			const uint64_t promised = ((uint64_t)it.info.total_values + bl - 1) / bl, possible = blocks_possible(it.info, it.len);
			s.want_blocks = std::min<uint64_t>(promised, it.max_blocks);
			L.blocks_wanted += s.want_blocks;
			/* a header that promises more blocks than the bytes can hold: the file is cut short.  Its walk would run out of data - unless the
			 * caller asks for fewer blocks than even these bytes could hold (acm_batch_index_blocks asks for exactly that many) */
			can_hold = promised <= possible || s.want_blocks < possible;
		}
		/* The device takes a stream that can be clean: an ACM file with room for marks whose bytes can hold the blocks it is asked for
		 * (one that cannot ends early, and how it ends is the host reader's to say), inside the walk's 32-bit arithmetic */
		s.on_dev = it.ok && it.has_marks && s.want_blocks >= 1 && can_hold &&
			   acmk_parse_supported(it.info.level, it.info.rows, it.len, s.want_blocks);
		if (!s.on_dev) {
			L.host_ids.push_back(i);
			continue;
		}
		const uint64_t slot = file_slot_bytes(it.len), nmarks = s.want_blocks + 1;
		const uint64_t cost = slot + nmarks * sizeof(acm_block_mark);
		const uint64_t held = g.file_bytes + g.marks * sizeof(acm_block_mark);
		if (g.k_last > g.k_first && (held + cost > budget || g.k_last - g.k_first >= ACM_PARSE_RANGE_MAX_STREAMS))
			close_group();
		s.group = L.groups.size();
		s.file_off = g.file_bytes;
		s.mark_off = g.marks;
		g.file_bytes += slot;
		g.marks += nmarks;
		g.k_last++;
		AcmParseJob j{};
		j.file_off = s.file_off;
		j.hdr_off = s.mark_off;
		j.file_len = (uint32_t)it.len;
		j.data_start = (uint32_t)it.info.header_bytes;
		j.level = it.info.level;
		j.rows = it.info.rows;
		j.blocks = (uint32_t)s.want_blocks;
		L.dev_ids.push_back(i);
		L.jobs.push_back(j);
	}
	close_group();
}

} // namespace acmbatch

extern "C" int acmk_index_layout_visit(const acm_stage_info *info, const uint64_t *len, const uint64_t *max_blocks, const uint8_t *ok,
				       const uint8_t *has_marks, size_t n, uint64_t budget, acmk_index_layout_visit_fn visit, void *ctx)
{
	using namespace acmbatch;
	std::vector<IndexItem> items(n);
	for (size_t i = 0; i < n; i++) {
		items[i].info = info[i];
		items[i].len = len[i];
		items[i].max_blocks = max_blocks[i];
		items[i].ok = ok[i] != 0;
		items[i].has_marks = has_marks[i] != 0;
	}
	IndexLayout L;
	acm_index_layout(items.data(), n, budget, &L);
	std::vector<uint64_t> w;
	for (const IndexSlot &s : L.slots)
		w.insert(w.end(), { s.want_blocks, s.file_off, s.mark_off, s.group, (uint64_t)s.on_dev });
	if (!w.empty())
		visit(ctx, "slots", w.data(), 5 * sizeof(uint64_t), L.slots.size());
	w.clear();
	for (const IndexGroup &g : L.groups)
		w.insert(w.end(), { (uint64_t)g.k_first, (uint64_t)g.k_last, g.file_bytes, g.marks });
	if (!w.empty())
		visit(ctx, "groups", w.data(), 4 * sizeof(uint64_t), L.groups.size());
	auto ids = [&](const char *name, const std::vector<size_t> &v) {
		std::vector<uint64_t> u(v.begin(), v.end());
		if (!u.empty())
			visit(ctx, name, u.data(), sizeof(uint64_t), u.size());
	};
	ids("dev_ids", L.dev_ids);
	ids("host_ids", L.host_ids);
	if (!L.jobs.empty())
		visit(ctx, "jobs", L.jobs.data(), sizeof(AcmParseJob), L.jobs.size());
	const uint64_t totals[] = { L.half_file_bytes, L.half_marks, (uint64_t)L.half_jobs, L.blocks_wanted };
	visit(ctx, "totals", totals, sizeof(uint64_t), sizeof(totals) / sizeof(totals[0]));
	return ACMHIP_OK;
}
