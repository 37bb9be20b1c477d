/*
 * acm_window_layout.h - where everything of a windowed batch decode goes (acm_batch_windows.cpp), decided on the host from the
 * headers, the file lengths, the block indices and the options alone.  Internal.  Neither this header nor acm_window_layout.cpp
 * knows a device (tests/test_window_layout.py); the driver walks a WindowLayout it never modifies.
 */
#ifndef ACM_WINDOW_LAYOUT_H
#define ACM_WINDOW_LAYOUT_H

#include <vector>

#include "acm_batch_layout.h"
#include "acm_device.h"
#include "libacm.h"

namespace acmbatch {

class Pool;     /* acm_pool.h */

/* ACM_BATCH_PARSE_AUTO: device parsing from this many staged blocks per call on.  Measured on an MI355X with 16 host threads
 * (profiles/window_decode_notes.txt): the device path pays ~0.15 ms more per call - a second round trip for the walk's results -
 * and ~1.3 us less per block */
constexpr uint64_t ACM_WINDOWS_AUTO_BLOCKS = 256;

/* samples a window delivers, given how many the stream has */
inline uint64_t window_words(uint64_t whole, uint64_t first, uint64_t max_words)
{
	return first >= whole ? 0 : std::min(max_words, whole - first);
}
/* the int16 rows of a window's `nb` staged blocks, in words: what its slice of the index arenas holds and a host-staged window uploads */
inline uint64_t window_rows_words(const acm_stage_info &info, uint32_t nb) { return (uint64_t)nb * info.rows * info.cols; }
/* the window's slot of the PCM arena: the `lead` samples of its first row in front of the first one wanted + the samples wanted */
inline uint64_t window_slot_words(uint64_t lead, uint64_t words) { return round_up(lead + words, 64); }

/* what the layout is computed from, per item: the probed header, the file length, and what the driver made of its index - whether
 * the file is ACM with an index it can have, what a window that reaches the end of the stream reports, the words acm_batch_decode
 * delivers for it.  marks[0 .. blocks] is read for the windows of an item that is ok only.  The layout itself never consults `ok`: an
 * item that is not ok has whole == 0, so none of its windows has samples */
struct WindowItem {
	acm_stage_info info{};
	uint64_t len = 0;
	bool ok = false;
	int32_t end_status = 0;
	uint64_t whole = 0;
	const acm_block_mark *marks = nullptr;
	uint32_t blocks = 0;
};

struct WindowSlot {
	/* what the caller's acm_batch_window receives */
	int32_t status = 0;
	uint64_t words = 0, slot_off = 0, slot_words = 0, dev_off = 0;
	/* the driver's */
	bool active = false;            /* has samples to decode */
	bool on_device = false;         /* staged by the device parser */
	uint32_t b0 = 0, nb = 0;        /* blocks staged: [b0, b0 + nb) */
	uint32_t row_begin = 0;         /* row of the first sample, counted from block b0 */
	uint64_t lead = 0;              /* samples of that row in front of the first one wanted */
	uint64_t idx_off = 0, hdr_off = 0, col_off = 0;
	uint64_t span_lo = 0, span_len = 0, file_off = 0;       /* device parsing: bytes [span_lo, span_lo + span_len) of the file, and their place */
};

struct WindowLayout {
	std::vector<WindowSlot> slots;
	std::vector<size_t> act;                /* windows with samples to decode, ascending */
	std::vector<size_t> dev_ids;            /* ... those the device parser takes */
	std::vector<size_t> host_ids;           /* ... and those the host stages from the start */
	std::vector<AcmParseJob> jobs;          /* [a]: the device parser's job for window dev_ids[a]; its file is the byte span of its blocks */
	std::vector<AcmBlockJob> bjobs;         /* every block of every job, window after window */
	uint64_t idx_total = 0, hdr_total = 0, pcm_total = 0, cols_total = 0, files_total = 0, max_columns = 0;
	uint64_t blocks_parsed = 0;             /* over every active window, whichever side parses it */
	/* the H_JOBS / D_JOBS arena: the jobs, the block jobs (each table padded to 64 bytes), then the results and their flags */
	size_t jobs_bytes = 0, bjobs_bytes = 0, res_bytes = 0;
	size_t bjobs_off() const { return jobs_bytes; }
	size_t res_off() const { return jobs_bytes + bjobs_bytes; }            /* = the bytes of the two tables that travel up */
	size_t job_arena_bytes() const { return jobs_bytes + bjobs_bytes + res_bytes; }
	bool dev_parse = false;                 /* opts.parse resolved */
};

/* ACMHIP_OK, or ACMHIP_ERR_ARG: opts.d_pcm too small, or more device windows or block headers than 32 bits count.  `out` is a fresh
 * WindowLayout whose slots are filled in either case (a refused call has told its windows their status and slots).  pool (may be null):
 * the job records - one per block of every device window - are filled through it, window by window, instead of by the caller alone */
int acm_window_layout(const WindowItem *items, size_t n, const acm_batch_window *wins, size_t nwin, const acm_batch_opts &opts, WindowLayout *out,
		      Pool *pool = nullptr);

} // namespace acmbatch

extern "C" {
/* The layout shown to a visitor, table by table (tests), as uint64 words unless said otherwise: "slots" (17 words per window: status
 * (sign-extended), words, slot_off, slot_words, dev_off, active, on_device, b0, nb, row_begin, lead, idx_off, hdr_off, col_off, span_lo,
 * span_len, file_off), "act", "dev_ids", "host_ids", "jobs" (AcmParseJob), "bjobs" (AcmBlockJob), then "totals": idx_total, hdr_total,
 * pcm_total, cols_total, files_total, max_columns, blocks_parsed, jobs_bytes, bjobs_bytes, res_bytes, dev_parse and the return code.
 * An item is info[i], len[i], ok[i], end_status[i], whole[i], marks[i] (blocks[i] + 1 entries; may be null), blocks[i]; a window is
 * three words of win3: item, first_word, max_words.  Returns acm_window_layout's code; a refused layout has slots, ids and totals, no jobs */
typedef void (*acmk_window_layout_visit_fn)(void *ctx, const char *table, const void *data, size_t elem_bytes, size_t count);
int acmk_window_layout_visit(const acm_stage_info *info, const uint64_t *len, const uint8_t *ok, const int32_t *end_status, const uint64_t *whole,
			     const acm_block_mark *const *marks, const uint32_t *blocks, size_t n, const uint64_t *win3, size_t nwin,
			     const acm_batch_opts *opts, acmk_window_layout_visit_fn visit, void *ctx);
}

#endif
