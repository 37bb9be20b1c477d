/*
 * acm_index_layout.h - where everything of a batch index build goes (acm_batch_index.cpp), decided on the host from the headers,
 * the file lengths and the room the caller gave alone.  Internal.  Neither this header nor acm_index_layout.cpp knows a device
 * (tests/test_index_layout.py); the driver walks an IndexLayout it never modifies.
 */
#ifndef ACM_INDEX_LAYOUT_H
#define ACM_INDEX_LAYOUT_H

#include <vector>

#include "acm_batch_layout.h"
#include "acm_device.h"

namespace acmbatch {

/* opts->max_group_bytes == 0.  The walk of a group takes as long as its longest stream almost however many streams it has (one wavefront each),
 * and the upload a group could hide is short: every further group costs that latency again.  Groups bound the memory, they do not add speed
 * (profiles/index_build_notes.txt: 1024 streams of 2 Msamples in 1 / 2 / 4 / 8 groups 69 / 95 / 167 / 310 ms) */
constexpr uint64_t ACM_INDEX_GROUP_BYTES = 1ull << 30;

/* what the layout is computed from, per item: the probed header, whether the probe took the file, its length, the marks the caller
 * has room for (has_marks: a buffer at all) */
struct IndexItem {
	acm_stage_info info{};
	uint64_t len = 0, max_blocks = 0;
	bool ok = false, has_marks = false;
};

struct IndexSlot {
	uint64_t want_blocks = 0;       /* blocks acm_index_file goes for: what the header promises, capped by max_blocks */
	uint64_t file_off = 0;          /* bytes from the start of its group's half of the file arenas; multiple of 16 */
	uint64_t mark_off = 0;          /* marks from the start of its group's half of the mark arenas: want_blocks + 1 entries */
	uint64_t group = 0;
	bool on_dev = false;
};

/* a run of streams that is on the device as one unit: one upload, one launch, one read-back */
struct IndexGroup {
	size_t k_first = 0, k_last = 0;         /* indices into dev_ids: [k_first, k_last) */
	uint64_t file_bytes = 0;                /* its file slots, back to back */
	uint64_t marks = 0;                     /* its mark entries */
};

struct IndexLayout {
	std::vector<IndexSlot> slots;
	std::vector<IndexGroup> groups;
	std::vector<size_t> dev_ids;            /* items the device walks, in group order */
	std::vector<size_t> host_ids;           /* items acm_index_file runs on from the start */
	std::vector<AcmParseJob> jobs;          /* [k]: the walk's job for item dev_ids[k]; offsets count from its group's halves */
	/* the halves of the arenas: the largest group's needs */
	uint64_t half_file_bytes = 0, half_marks = 0;
	size_t half_jobs = 0;
	uint64_t blocks_wanted = 0;             /* over every item */
};

/* budget: file bytes + mark bytes of a group (0: ACM_INDEX_GROUP_BYTES); a single file above it is a group of its own */
void acm_index_layout(const IndexItem *items, size_t n, uint64_t budget, IndexLayout *out);

} // namespace acmbatch

extern "C" {
/* The layout shown to a visitor, table by table (tests), as uint64 words unless said otherwise: "slots" (5 words per item: want_blocks,
 * file_off, mark_off, group, on_dev), "groups" (4 words: k_first, k_last, file_bytes, marks), "dev_ids", "host_ids", "jobs" (AcmParseJob),
 * then "totals": half_file_bytes, half_marks, half_jobs, blocks_wanted.  An item is info[i], len[i], max_blocks[i], ok[i], has_marks[i]. */
typedef void (*acmk_index_layout_visit_fn)(void *ctx, const char *table, const void *data, size_t elem_bytes, size_t count);
int acmk_index_layout_visit(const acm_stage_info *info, const uint64_t *len, const uint64_t *max_blocks, const uint8_t *ok,
			    const uint8_t *has_marks, size_t n, uint64_t budget, acmk_index_layout_visit_fn visit, void *ctx);
}

#endif
