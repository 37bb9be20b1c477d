/*
 * acm_dense_layout.h - the device-free half of acm_batch_decode_windows_dense (acm_batch_windows.cpp): whether the call is one the
 * dense writer takes, which windows it turns away softly, how large the output is, and - once staging has settled what every
 * window delivers - the tables the gather kernel reads and which of the four kernels that is (acm_dense_tables).  Internal.
 * Neither this header nor acm_dense_layout.cpp knows a device (tests/test_dense_crops.py); where a window's samples sit in the
 * intermediate arena stays acm_window_layout.cpp's.
 */
#ifndef ACM_DENSE_LAYOUT_H
#define ACM_DENSE_LAYOUT_H

#include <vector>

#include "acm_resample_layout.h"
#include "acm_window_layout.h"

namespace acmbatch {

/* samples the intermediate PCM arena is asked for beyond the windows' slots.  The gather kernel needs none: it loads only aligned
 * 16-byte lines that hold a sample of the window, and a slot is a whole number of 128-byte runs of a 256-byte aligned arena.  One
 * slot of slack keeps a slip in that arithmetic inside memory the call owns */
constexpr uint64_t ACM_DENSE_PCM_SLACK = 64;

struct DenseLayout {
	uint64_t frames = 0, row_words = 0;     /* T, and R = T * channels */
	uint32_t channels = 0;
	bool planar = false, f32 = false;
	uint64_t out_words = 0;                 /* nwin * R: what opts->d_pcm must hold, in samples of the output type */
	std::vector<acm_batch_window> wins;     /* the windows as acm_window_layout gets them: one turned away asks for no samples */
	std::vector<uint8_t> rejected;          /* [k]: window k's item has another channel count than the batch (no ACM_DENSE_MIX) */
	bool mix = false;                       /* ACM_DENSE_MIX: such a window is decoded and converted instead */
	std::vector<uint8_t> mode;              /* [k]: AcmDenseMode - what row k does with its window's samples, if it gets any */
	bool resample = false;                  /* ACM_DENSE_RESAMPLE: a window of a file at another rate than `rate` is resampled */
	uint32_t rate = 0;
	std::vector<uint8_t> bad_ratio;         /* [k]: turned away for its item's rate (also counted in `rejected`) */
	std::vector<int8_t> ratio;              /* [k]: which of `tables` row k is filtered by if it gets samples, or -1; empty without a table */
	std::vector<uint8_t> chans;             /* [k]: samples per source frame of a row that is filtered */
	std::vector<std::shared_ptr<const ResampleTable>> tables;      /* the distinct tables of the call, in the order of their first window */
	std::vector<uint32_t> table_rate;       /* [id]: the rate of the file whose window brought table id in */
	bool speed = false;                     /* ACM_DENSE_SPEED: a window's `reserved` is its speed, and a ratio beyond the exact table is wide */
	std::vector<SpeedFilter> filt;          /* [k]: L, M and the filter form of a row that is filtered; empty without a table */
	bool has_wide() const
	{
		for (const auto &t : tables)
			if (t->wide)
				return true;
		return false;
	}
	acm_batch_opts inner{};                 /* the options of the windowed decode underneath: int16 rows into the handle's own arena */
	uint64_t pcm_arena_words(uint64_t pcm_total) const { return pcm_total + ACM_DENSE_PCM_SLACK; }
	/* the row table travels behind the device parser's tables in the H_JOBS / D_JOBS arenas: where, the map of acm_dense_call.h says */
	size_t table_off(const WindowLayout &L) const;
	/* ... and, where a window may be resampled, the second table and the ratios' taps behind it, each from a multiple of 16 bytes on */
	size_t row_table_bytes() const { return wins.size() * sizeof(AcmDenseRow); }
	size_t resample_off() const { return row_table_bytes(); }
	/* (a call that may have a wide row keeps room for the larger records of acm_dense_speed.hip) */
	size_t second_bytes() const { return has_wide() ? sizeof(AcmSpeedRow) : sizeof(AcmResampleRow); }
	size_t taps_off() const { return resample_off() + wins.size() * second_bytes(); }
	size_t tap_words(size_t id) const { return (size_t)round_up(tables[id]->q.size(), 8); }
	size_t tap_at(size_t id) const
	{
		size_t at = 0;
		for (size_t i = 0; i < id; i++)
			at += tap_words(i);
		return at;
	}
	size_t table_bytes() const { return tables.empty() ? row_table_bytes() : taps_off() + tap_at(tables.size()) * sizeof(int16_t); }
};

/* ACMHIP_OK, or ACMHIP_ERR_ARG for a call the dense writer refuses as a whole (include/acm_hip.h) - then nothing of `out` is to be
 * used.  opts: the caller's, defaults filled in */
int acm_dense_prepare(const WindowItem *items, size_t n, const acm_batch_window *wins, size_t nwin, const acm_batch_opts &opts,
		      const acm_dense_opts *dense, DenseLayout *out);

/* what the caller's window k receives, from its slot of the layout underneath */
void acm_dense_report(const DenseLayout &D, const WindowSlot &s, size_t k, acm_batch_window *w);

/* Which kernel takes the gather launch, and how much of the table region goes up with it - decided here, once, by what staging left of
 * every window: final[k].words is what window k delivers (0: the host stager turned it away).  `table`: table_bytes() of the jobs
 * arena, 16-byte aligned.  The row table is always filled and goes up; the second table (at resample_off()) and the taps (at taps_off())
 * go up with it for DENSE_RESAMPLE - AcmResampleRow records - and DENSE_SPEED - AcmSpeedRow records -, the kernels that read them */
enum DenseKernel {
	DENSE_PLAIN = 0,        /* acm_dense_rows: no row converts, none is filtered */
	DENSE_MIXED = 1,        /* acm_dense_mixed: a row converts between mono and stereo (ACM_DENSE_MIX) */
	DENSE_RESAMPLE = 2,     /* acm_dense_resample: a row that got samples is filtered (ACM_DENSE_RESAMPLE), by the exact filter */
	DENSE_SPEED = 3,        /* acm_dense_speed: ... by the wide one (ACM_DENSE_SPEED) */
};
struct DenseLaunch {
	DenseKernel kernel;
	size_t bytes;           /* of `table`, from its start */
};
DenseLaunch acm_dense_tables(const DenseLayout &D, const WindowSlot *slots, const acm_batch_window *final, uint8_t *table);

/* Its steps.  The row table; returns whether a row converts - else the table is, bit for bit, what a call without ACM_DENSE_MIX makes */
bool acm_dense_rows(const DenseLayout &D, const WindowSlot *slots, const acm_batch_window *final, AcmDenseRow *rows);
/* ACM_DENSE_RESAMPLE, for a layout with tables: the second table, from the first one (a row that got no samples is not filtered), and
 * the taps behind it (tap_at(tables.size()) words).  Returns whether a row is filtered */
bool acm_dense_resample_rows(const DenseLayout &D, const AcmDenseRow *rows, AcmResampleRow *rs, int16_t *taps);
/* ACM_DENSE_SPEED: whether a row that got samples takes the wide filter, and the second table and the taps of a call in which one does */
bool acm_dense_wide_rows(const DenseLayout &D, const AcmDenseRow *rows);
void acm_dense_speed_rows(const DenseLayout &D, const AcmDenseRow *rows, AcmSpeedRow *sp, int16_t *taps);

} // namespace acmbatch

extern "C" {
/* The dense layout shown to a visitor (tests).  Items, windows and the visitor as in acmk_window_layout_visit; final_words (may be
 * null: what the window layout says) stands for what staging left of every window.  A refused call visits "totals" alone.  Tables,
 * as uint64 words: "wins" (3 per window: item, first_word, max_words as the window layout gets them), "rejected", "report" (5 per
 * window: status (sign-extended), words, dev_off, slot_off, slot_words as the caller receives them), "rows" (2 per window: src,
 * count), with ACM_DENSE_MIX alone "mix" (nwin + 1 words: AcmDenseMode per window, then 1 if a row converts, else 0), with
 * ACM_DENSE_RESAMPLE alone "resample" (5 per window: L, M, the ratio's number in "tables" or all ones, the row's frames, 1 if the window
 * is turned away for its rate; L = M = 1 for a row that is not filtered, 0 for one turned away; nwin + 1 entries, the last one's first
 * word 1 if a row is filtered) and "tables" (6 per distinct ratio: rate_in, L, M, K, Wd, where its taps begin behind the tables), "totals":
 * frames, row_words, channels, planar, f32, out_words, pcm_arena_words, blocks_parsed, table_off, table_bytes and the return code */
int acmk_dense_layout_visit(const acm_stage_info *info, const uint64_t *len, const uint8_t *ok, const int32_t *end_status, const uint64_t *whole,
			    const acm_block_mark *const *marks, const uint32_t *blocks, size_t n, const uint64_t *win3, size_t nwin,
			    const acm_batch_opts *opts, const acm_dense_opts *dense, const uint64_t *final_words,
			    acmk_window_layout_visit_fn visit, void *ctx);
/* The same with speeds[k] (may be null: zeros) as window k's acm_batch_window.reserved.  With ACM_DENSE_SPEED, in place of "resample"
 * and "tables": "speed" (8 per window: the kind - 0 not filtered, 1 exact, 2 wide, all ones turned away for its ratio -, L, M, the
 * table's number in "speed_tables" or all ones, the row's frames, step, b, Wd; nwin + 1 entries, the last one's first word what the
 * launch is: 0 the kernel of a call without the flags, 1 acm_dense_resample, 2 acm_dense_speed) and "speed_tables" (8 per distinct
 * table: 1 if wide, c, L, M, K, Wd, phases, where its taps begin) */
int acmk_dense_speed_layout_visit(const acm_stage_info *info, const uint64_t *len, const uint8_t *ok, const int32_t *end_status,
				  const uint64_t *whole, const acm_block_mark *const *marks, const uint32_t *blocks, size_t n, const uint64_t *win3,
				  const uint32_t *speeds, size_t nwin, const acm_batch_opts *opts, const acm_dense_opts *dense,
				  const uint64_t *final_words, acmk_window_layout_visit_fn visit, void *ctx);
}

#endif
