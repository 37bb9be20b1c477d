/*
 * acm_device.h - structures shared between the launch planner (host) and the
 * HIP kernels.  Internal; the public boundary is include/acm_hip.h.
 */
#ifndef ACM_DEVICE_H
#define ACM_DEVICE_H

#include <stdint.h>

#include "acm_hip.h"

/* per-stream record as the kernels see it */
struct AcmDevStream {
	uint64_t idx_off;      /* int16 units to staged row 0 */
	uint64_t hdr_off;      /* blkhdr units to block 0 */
	uint64_t pcm_off;      /* int16 units to the first emitted sample */
	uint64_t n_emit;       /* samples to emit from row_begin*cols */
	uint64_t scratch_off;  /* stage-wise path: int32 units into the scratch planes */
	uint32_t level;
	uint32_t rows;
	uint32_t nrows;        /* staged rows present */
	uint32_t row_begin;    /* first emitted row */
	uint32_t halo_row;     /* first staged row the kernels read: max(row_begin-2, 0) */
	uint32_t pad;
};

/* one workgroup of the fused kernel: `T` payload rows starting at row0 */
struct AcmTile {
	uint32_t stream;
	int32_t row0;          /* first payload row (a carry-mode lead-in tile may start before row 0) */
	uint32_t flags;        /* ACM_TILE_*: carry-mode kernels only */
	uint32_t pad;
};
/* carry mode: consecutive tiles of a stream hand the tail of every pass's input to the next tile through LDS instead
 * of recomputing two halo rows; a workgroup walks a contiguous run of the tile table */
#define ACM_TILE_FRESH   1u    /* nothing in front of this tile: the carries start from zero (stream row 0, or a lead-in) */
#define ACM_TILE_DISCARD 2u    /* lead-in: run the passes to build the carries, store no PCM */
/* records of the chunk kernel whose chunks are ONE row (acm_chunk, level 11) */
#define ACM_TILE_ROW1    4u    /* the chunk is row 1 of its stream: one row in front of it */
#define ACM_TILE_ODD     8u    /* the chunk starts on the second row of a pair (idx_off still names the entry of the pair in front of that pair) */
#define ACM_TILE_ONEBLOCK 16u  /* chunk records: every row in reach of the chunk - the two in front of it through its last - lies in ONE block
                                * (hdr_blk), so one val scales them all (decode.c:586-600: val is per block).  Geometry only: the planner
                                * knows it without looking at a header; acm_chunk takes its fast path on it */

/* one tile of the lean kernels (acm_tile2, acm_chunk): tile_rows consecutive rows of a stream, all of them present and emitted.
 * Tiles of a stream are consecutive table entries; the first one carries ACM_TILE_FRESH when it is the stream's row 0 - or, for a
 * window into a stream (rows from a tile boundary on), it is a record of the tile IN FRONT of the window carrying ACM_TILE_DISCARD:
 * decoded like any other to build the carries, its PCM dropped. */
struct AcmTile2 {
	uint64_t idx_off;      /* int16 units: staged index of (tile row 0, column 0) */
	uint64_t pcm_off;      /* int16 units: where sample (tile row 0, column 0) goes */
	uint32_t hdr_blk;      /* blkhdr index of the block that holds tile row -2 (tile row 0 in a stream's first tile) */
	uint32_t rowpos;       /* position of that row inside its block */
	uint32_t magic;        /* ceil(2^32 / acm_rows); 0 for acm_rows == 1 */
	uint32_t flags;        /* ACM_TILE_FRESH */
};

/* resolved H1 patch for the stage-wise path: scratch[dst] = value */
struct AcmDevPatch {
	uint64_t dst;
	int32_t value;
	uint32_t pad;
};

/* device-side bit parsing (acm_parse.hip): one stream = one lane */
struct AcmParseJob {
	uint64_t file_off;     /* bytes into the file arena; multiple of 16, >= 16 zero bytes behind every file */
	uint64_t idx_off;      /* int16 units into the staged-index arenas */
	uint64_t hdr_off;      /* blkhdr units */
	uint64_t col_off;      /* uint32 units into the column-offset arena (blocks * cols entries per stream) */
	uint32_t file_len;     /* bytes */
	uint32_t data_start;   /* first bitstream byte (14, or 42 behind a WAVC prefix) */
	uint32_t level;
	uint32_t rows;
	uint32_t blocks;       /* blocks to parse */
	uint32_t range_unit;   /* block ranges of this stream are cut at multiples of this many blocks (0 / 1: anywhere): acmk_range_bound */
	/* byte-plane staging by the device parser (the chunk kernel's form: levels whose acmk_tile2m_stages is 6): rows
	 * [0, mf_rows) of the stream are written into the byte-plane arena at mf_off (bytes; the pair of zeros first), their pair-table
	 * entries from mf_pair_off on; only the rows from mf_rows - 2 on are written to the int16 arena.  mf_rows = 0: int16 throughout */
	uint64_t mf_off;
	uint32_t mf_pair_off;
	uint32_t mf_rows;
};
struct AcmParseResult {
	uint32_t blocks_done;
	uint32_t status;       /* 0 = the scan walked every block it was asked for; else the host must re-parse this stream */
	uint32_t end_bit;      /* bit offset behind the last block walked: where the next block range of the stream resumes */
	uint32_t mf_at;        /* ... and where its next block starts in the stream's byte-plane region, in 64-byte units (width from pwr) */
};

/* indexed input (acm_parse_scan_blocks): block `block` of job `job` is a walk of its own - from `bit` (relative to the job's file_off),
 * where its 20-bit header must read h20 (val << 4 | pwr, as the bitstream holds it), to exactly end_bit.  Written by the host from a
 * block index it has checked: bit + 20 <= end_bit <= 8 * the job's file_len */
struct AcmBlockJob {
	uint32_t job;
	uint32_t block;
	uint32_t bit;
	uint32_t end_bit;
	uint32_t h20;
	uint32_t pad;
};

/* dense crop batches (acm_dense.hip): row k of the output is `count` samples from sample `src` of the int16 PCM arena on, zeros behind them */
struct AcmDenseRow {
	uint64_t src;
	uint64_t count;        /* 0: the row is all zeros and src is not read */
};
/* ACM_DENSE_MIX (acm_dense_mix.hip): what a row does with its source samples.  A converting row carries its mode in the bits of
 * `count` from ACM_DENSE_MODE_SHIFT on, and `count` is then the SOURCE samples; a row that copies or splits has none of them set, so
 * the table of a call in which nothing converts is the one acm_dense_rows reads */
enum AcmDenseMode {
	ACM_DENSE_MODE_COPY = 0,        /* the item has the batch's channel count, rows interleaved (or mono) */
	ACM_DENSE_MODE_SPLIT = 1,       /* ... stereo rows as a plane per channel */
	ACM_DENSE_MODE_DOWN = 2,        /* stereo item, mono batch: (L + R) >> 1 */
	ACM_DENSE_MODE_UP_INTER = 3,    /* mono item, stereo batch, interleaved: the sample in both channels */
	ACM_DENSE_MODE_UP_PLANAR = 4,   /* mono item, stereo batch, planar: the sample in both planes */
};
#define ACM_DENSE_MODE_SHIFT 56
#define ACM_DENSE_COUNT_MASK ((1ull << ACM_DENSE_MODE_SHIFT) - 1)
/* ACM_DENSE_RESAMPLE (acm_dense_resample.hip): a second table beside the first, one record per row.  L == 0: the row is written as
 * its AcmDenseRow says.  Else that record names the row's SOURCE samples and its channel conversion as ever, and the row is the
 * `frames_in` frames they make, filtered into n_out frames by the ratio's Q14 table: L phases of 2 * Wd taps from int16 `tab` of the
 * tap arena on (a multiple of 8) */
struct AcmResampleRow {
	uint32_t tab, L, M, Wd;
	uint64_t n_out, frames_in;
};
/* ACM_DENSE_SPEED (acm_dense_speed.hip): that record for a call in which some row takes the wide filter.  wide == 0: the record's
 * head is the row's AcmResampleRow.  Else the table at `tab` has (1 << b) + 1 phases of 2 * Wd taps, and output frame j reads from
 * source position j * step in 32.32 fixed point (include/acm_hip.h) */
struct AcmSpeedRow {
	uint32_t tab, L, M, Wd;
	uint64_t n_out, frames_in;
	uint64_t step;
	uint32_t b, wide;
};
/* acm_batch_decode_windows_overlay (acm_dense_overlay.hip): output row r is source row a of the source arena, with source row b laid
 * over it (b == ACM_OVERLAY_NONE: nothing is) and the sum scaled by vol (Q12, never 0 here).  snr != 0: b's gain is made from the
 * two rows' energies (include/acm_hip.h), else it is `gain` */
struct AcmOverlayRow {
	uint32_t a, b, vol, snr, gain, pad;
};
/* ... and what the combine launch leaves per output row: the gain used and the energies it was made from (0 where none was) */
struct AcmOverlayResult {
	uint64_t gain, energy_a, energy_b;
};
/* acm_batch_decode_windows_overlay_fir (acm_dense_fir.hip): row dst of the source arena is row src filtered, channel by channel:
 * y[j] = clamp((sum over u < nblk * ACM_FIR_TAP_BLOCK of g[u] * x[j + lead + u] + half) >> shift), g the response reversed and
 * zero-padded to whole tap blocks (acm_fir_layout.cpp), as pairs of int16 from dword taps_off of the call's taps on; lead <= 0 */
#define ACM_FIR_TAP_BLOCK 64u
struct AcmFirRow {
	uint32_t src, dst, taps_off, nblk;
	int32_t lead;
	uint32_t shift;
};
/* acm_batch_decode_windows_features (acm_dense_feat.hip): the bank as the feature kernel reads it - device pointers to the uploaded
 * tables (acm_feat_layout.h: the window on a multiple of 16 bytes) and to the DFT's B operand acm_feat_twiddle made of cs */
struct AcmFeatDesc {
	uint32_t n_fft, hop, n_mels, flags;
	const int16_t *window;
	const uint16_t *mel_first, *mel_count;
	const uint32_t *mel_off;
	const uint16_t *mel_w;
	const void *twiddle;
	/* acm_batch_decode_windows_logmel (acmk_launch_dense_logmel; acmk_launch_dense_feat reads none of it): acm_feat_log's fields, and
	 * with ACM_FEAT_LOG_TOP the rows' maxima, nrows int32 the launcher resets */
	uint32_t log_flags;
	int32_t floor_q16;
	uint32_t mul_q24;
	int32_t offset_q16;
	uint32_t top_q16;
	int32_t *rowmax;
};

/* levels the fused tile kernel covers; its tile geometry, like every kernel's, is owned by acm_kernel_geo.h (acmk_fused_tile_rows) */
#define ACM_K1_MIN_LEVEL 5
#define ACM_K1_MAX_LEVEL 12
/* levels the lean tile kernel (acm_tile2) covers (measured: 32 KB tiles lose to the 64-128 KB tiles of acm_fused_tile from level 10 on) */
#define ACM_K2_MIN_LEVEL 6
#define ACM_K2_MAX_LEVEL 14
/* levels whose acm_tile2 tiles have a packed staged form and a kernel build that reads it (acm_tile2p): the 32 KB tiles of four
 * workgroups per CU whose two-row stage-0 history fits LDS beside the tile */
#define ACM_K2P_MIN_LEVEL 6
#define ACM_K2P_MAX_LEVEL 9
/* levels whose acm_tile2 build has a three-stage first pass and therefore a build that runs it on the matrix cores, fed with the
 * byte-plane staged form (acmhip_mform_rows) */
#define ACM_K2M_MIN_LEVEL 7
#define ACM_K2M_MAX_LEVEL 14
/* levels below that (cols <= 16) have their own one-launch kernel: the cascade fits one thread's registers */
#define ACM_SMALL_MAX_LEVEL 4

/* Kernel-selection and tuning switches are read from the environment only in -DACM_TUNING builds (profiles/build_variant.sh,
 * ACM_TUNING=1 python -c 'from libacm_amd import _build; _build.build_hip(True)'): what a drop-in library does must not depend on
 * its caller's environment (Weak 9).  The shipped library honours ACM_HIP_DEVICE, ACM_BATCH_TRACE and acmtool's ACMTOOL_*;
 * everything else is a plan / batch flag of include/acm_hip.h. */
#ifdef ACM_TUNING
#include <stdlib.h>
#define ACM_TUNING_ENV(name) getenv(name)
#else
#define ACM_TUNING_ENV(name) ((const char *)0)
#endif

#ifdef __cplusplus
extern "C" {
#endif
/* grow-only staging arenas owned by a device handle (acm_hip_api.cpp): pinned host slots first, device slots
 * from ACM_ARENA_D_IDX on.  hipHostMalloc of gigabytes costs ~0.1 s; the batch front end reuses them across
 * calls.  A device handle serves one batch at a time (acmhip_arena_lock/unlock bracket acm_batch_decode). */
enum {
	ACM_ARENA_H_IDX = 0, ACM_ARENA_H_HDR, ACM_ARENA_H_PCM, ACM_ARENA_H_FILES, ACM_ARENA_H_JOBS, ACM_ARENA_H_PKBLOB, ACM_ARENA_H_PKCHUNK,
	ACM_ARENA_D_IDX, ACM_ARENA_D_HDR, ACM_ARENA_D_PCM, ACM_ARENA_D_FILES, ACM_ARENA_D_COLPOS, ACM_ARENA_D_JOBS, ACM_ARENA_D_STAGE,
	ACM_ARENA_D_PKBLOB, ACM_ARENA_D_PKCHUNK, ACM_ARENA_D_BLKOFF,
	ACM_ARENA_D_MARKS, ACM_ARENA_H_MARKS,           /* the marks of a batch index build's two groups (acm_batch_index.cpp), or of a decode that hands
	                                                   the index out (acm_batch_decode_indexed: hdr_total of them), on the device and pinned */
	ACM_ARENA_D_SRC,                                /* the source rows of acm_batch_decode_windows_overlay: int16 PCM, nwin rows of a dense call */
	ACM_ARENA_D_FEAT,                               /* acm_batch_decode_windows_features: the int16 rows its combine launch writes, and behind
	                                                   them the DFT's B operand (acm_feat_layout.h) */
	ACM_ARENA_SLOTS
};
/* is this slot pinned host memory (else device memory)? */
static inline int acm_arena_is_host(int slot) { return slot < ACM_ARENA_D_IDX || slot == ACM_ARENA_H_MARKS; }
int acmhip_arena_get(acmhip_device *dev, int slot, size_t bytes, void **out);
void acmhip_arena_lock(acmhip_device *dev);
void acmhip_arena_unlock(acmhip_device *dev);
int acmhip_copy_stream(acmhip_device *dev, void **out);          /* second stream for overlapped read-back */
#define ACM_AUX_STREAMS 2
int acmhip_aux_stream(acmhip_device *dev, int k, void **out);    /* batch pipeline: 0 = device bit parsing, 1 = file uploads */
int acmhip_report_hip(int hip_error, const char *what);
/* the handle's launch caps as they were set (0 in a field: the built-in value), for the callers of the launchers below; and the device-free
 * half of acmhip_device_set_launch_caps (acm_kernel_geo.cpp): checks `caps` (null: all built-in) against acm_launch_caps.h, then *previous = *held,
 * *held = *caps - or ACMHIP_ERR_ARG and nothing changed */
acmhip_launch_caps acmhip_device_launch_caps(const acmhip_device *dev);
int acmk_launch_caps_set(acmhip_launch_caps *held, const acmhip_launch_caps *caps, acmhip_launch_caps *previous);
void acmhip_set_error_text(const char *text);                    /* what acmhip_last_error() returns on this thread */          /* records the text, returns ACMHIP_ERR_HIP */

/* Two kinds of acmk_* functions.  The ones that launch nothing - a build's tile rows, threads, grid, first-pass depth, lead-in, packed
 * slots, the split of a chunk table, what the device parser accepts and where it cuts - live in acm_kernel_geo.cpp: plain C++ over the
 * tables of acm_kernel_geo.h, linkable without a device or a kernel.  The launchers (acmk_launch_*, acmk_warmup) live with their kernels in
 * acm_kernels.hip (acm_kernels_f32.hip: the _f32 ones), acm_parse.hip and the five acm_dense*.hip, and take block size and
 * grid from the queries - the dense ones from dense_geo() of acm_dense_geo.h, which is as device-free as the queries are.  `stream` is a hipStream_t.  fmt | ACMK_FMT_F32 (with the format bits 0): the float32 builds,
 * d_pcm (and d_sink) then hold floats and the streams' pcm_off / n_emit count them (acmhip_plan_launch_f32) */
#define ACMK_FMT_F32 0x100u
/* one number over every table of acm_kernel_geo.h, as the planner's half (acm_kernel_geo.cpp) and the kernels' half (acm_kernels.hip) of
 * the library were compiled: acmhip_device_open refuses a library in which they differ */
uint64_t acmk_geo_digest(void);
uint64_t acmk_geo_digest_kernels(void);
int acmk_tuning_build(void);                                     /* 1 if the library was built with -DACM_TUNING (its environment switches are live) */
int acmk_warmup(void *stream);                                   /* an empty launch: makes the runtime load the kernels' code object */
int acmk_fused_variants(void);                                   /* number of fused-kernel variants built in */
int acmk_fused_tile_rows(uint32_t level, int variant);           /* tile rows incl. the 2 halo rows, 0 if unsupported */
int acmk_fused_has_carry(uint32_t level, int variant);           /* does a carry-mode build of this geometry exist? */
int acmk_fused_threads(uint32_t level, int variant);             /* threads of a workgroup */
int acmk_fused_grid(uint32_t level, int variant, int cus);       /* persistent workgroups the launch uses at most */
int acmk_launch_fused(uint32_t level, int variant, int cus, int carry, const AcmDevStream *d_streams, const AcmTile *d_tiles,
		      uint32_t ntiles, const int16_t *d_idx, const acmhip_blkhdr *d_hdr, int16_t *d_pcm, unsigned fmt, void *stream);
int acmk_tile2_rows(uint32_t level);                            /* rows per acm_tile2 tile, 0 if the level is not covered */
int acmk_tile2_threads(uint32_t level);
int acmk_tile2_grid(uint32_t level, int cus);
#define ACM_K2_SINK_BYTES 65536                               /* >= one tile of PCM: where lead-in tiles put theirs */
#define ACM_K2_SINK_F32_BYTES (2 * ACM_K2_SINK_BYTES)         /* ... of float32 PCM */
int acmk_launch_tile2(uint32_t level, int cus, const AcmTile2 *d_tiles, uint32_t ntiles, const int16_t *d_idx, const acmhip_blkhdr *d_hdr, int16_t *d_pcm,
		      int16_t *d_sink, unsigned fmt, void *stream);
/* the packed staged form (include/acm_hip.h): same tiles as acm_tile2 (records with idx_off = the tile's first entry in the chunk table and
 * hdr_blk / rowpos naming the block of tile row 0), stage-0 inputs unpacked from chunks of one width class each */
int acmk_tile2p_rows(uint32_t level);                           /* rows per packed tile (= acmk_tile2_rows), 0 if the level has no packed build */
int acmk_tile2p_group_rows(uint32_t level);                     /* rows that share a width class per column pair */
int acmk_tile2p_slots(uint32_t level);                          /* chunk descriptors per tile: waves x descriptors per wave */
int acmk_tile2p_waves(uint32_t level);
int acmk_tile2p_pad_shift(uint32_t level);                      /* the tile's LDS rows carry one pad dword per 2^shift elements */
int acmk_tile2p_grid(uint32_t level, int cus);                  /* persistent workgroups of its launch at most */
int acmk_launch_tile2p(uint32_t level, int cus, const AcmTile2 *d_tiles, uint32_t ntiles, const acmhip_packed_chunk *d_chunks, const uint8_t *d_blob,
		       const acmhip_blkhdr *d_hdr, int16_t *d_pcm, int16_t *d_sink, unsigned fmt, void *stream);
/* the byte-plane staged form: the same tile records as acm_tile2 except that idx_off is the pair-table entry of the row pair in front of the tile */
int acmk_tile2m_rows(uint32_t level);                           /* = acmk_tile2_rows, 0 if the level has no such build */
int acmk_tile2m_threads(uint32_t level);
int acmk_tile2m_lead_in(uint32_t level);                        /* tiles of this build in front of a window into a stream (ACM_TILE_DISCARD records) */
int acmk_tile2m_run_waves(uint32_t level, int cus);             /* wavefronts that share a launch's table (the chunk kernel), else 0 */
/* how those W wavefronts share a table of ntiles chunks: wavefront w takes the chunks [w * static_per, (w + 1) * static_per) - below the
 * threshold (acm_kernel_geo.cpp states the rule) that is the whole table, static_per = ceil(ntiles / W), nclaimed = 0, as ever -, and the
 * chunks behind W * static_per are nclaimed runs of run_chunks (the last one may be shorter) which the wavefronts claim in ascending
 * order as they come free.  Device-free.  -1: the level has no chunk kernel */
int acmk_tile2m_split(uint32_t level, int cus, uint32_t ntiles, uint32_t *static_per, uint32_t *run_chunks, uint32_t *nclaimed);
/* process-wide policy of that split in place of the levels' compiled-in ones (tests, sweeps): chunks per claimed run (0: none are claimed)
 * and the static share in thousandths; a negative argument restores the default.  Hands back the values in force before (negative: default) */
void acmk_tile2m_claim_config(int run_chunks, int static_permille, int *old_run_chunks, int *old_static_permille);
int acmk_tile2m_grid(uint32_t level, int cus);                  /* persistent workgroups of its launch at most */
int acmk_tile2m_stages(uint32_t level);                         /* stages of the first pass of the build this process uses (3, 4 or 6): the form keeps 2^stages columns of a
                                                                 * residue class side by side, and acmk_launch_tile2m picks its kernel by it */
/* d_claim (the chunk kernel; null: the static split whatever the table's size): ONE zeroed word that the launch's wavefronts count their
 * claims in and leave at zero again.  Two launches that may run at the same time need a word each; launches on one stream - all launches of
 * a plan: it launches on its device's one stream - follow each other and share one */
int acmk_launch_tile2m(uint32_t level, int cus, const AcmTile2 *d_tiles, uint32_t ntiles, const uint8_t *d_mform, const acmhip_mform_pair *d_pairs,
		       const acmhip_blkhdr *d_hdr, int16_t *d_pcm, int16_t *d_sink, unsigned fmt, uint32_t *d_claim, void *stream);
/* list_slice (here and in the launchers of stream lists below), small_grid_x, parse_slice / parse_grid_x and dense_grid: the handle's launch caps
 * (acmhip_device_launch_caps, acm_launch_caps.h) as plain values; 0 = the built-in one */
int acmk_launch_unpack(const AcmDevStream *d_streams, const uint32_t *d_list, uint32_t nlist, uint64_t max_elems,
		       const int16_t *d_idx, const acmhip_blkhdr *d_hdr, int32_t *d_x, uint32_t shift, uint32_t list_slice, void *stream);
int acmk_launch_prefix(const AcmDevStream *d_streams, const uint32_t *d_list, uint32_t nlist, uint64_t max_elems,
		       uint32_t level, const int16_t *d_idx, const acmhip_blkhdr *d_hdr, int32_t *d_y, uint32_t list_slice, void *stream);   /* levels 13-15: unpack + level-12 stages */
int acmk_plane_tile_rows(void);                                 /* tile rows (incl. 2 halo rows) of the level-12 plane kernel */
int acmk_plane_threads(void);
int acmk_plane_grid(int cus);                                   /* persistent workgroups of that kernel */
int acmk_launch_fused_plane(int cus, int carry, const AcmDevStream *d_streams, const AcmTile *d_tiles, uint32_t ntiles,
			    const int32_t *d_plane, int16_t *d_pcm, unsigned fmt, void *stream);
int acmk_launch_patch(const AcmDevPatch *d_patches, uint64_t n, int32_t *d_x, void *stream);
int acmk_launch_stage(const AcmDevStream *d_streams, const uint32_t *d_list, uint32_t nlist, uint64_t max_elems,
		      uint32_t level, uint32_t k, const int32_t *d_in, int32_t *d_out, uint32_t shift, uint32_t list_slice, void *stream);
/* acm_parse.hip's launchers; acmk_parse_supported, acmk_stripe_bound and acmk_range_bound: acm_kernel_geo.cpp (acm_parse_bounds.h is the text
 * the kernels and the host share) */
int acmk_parse_supported(uint32_t level, uint32_t rows, uint64_t file_len, uint64_t blocks);
/* d_marks (here and in the two launchers below; may be null): the block index as a by-product of the walk (acm_batch_decode_indexed) - an arena
 * of acm_block_mark indexed like d_hdr; every block the walk completes leaves d_marks[hdr_off + b] = { its first bit, val, pwr }.  The entry
 * behind a stream's last block is not written: it is d_res[j].end_bit of a walk that came back clean */
int acmk_launch_parse(const AcmParseJob *d_jobs, uint32_t njobs, const uint8_t *d_files, uint32_t *d_colpos, int16_t *d_idx,
		      acmhip_blkhdr *d_hdr, AcmParseResult *d_res, uint32_t *d_flags, uint64_t max_columns, acm_block_mark *d_marks, uint32_t parse_slice, uint32_t parse_grid_x,
		      void *stream);
/* the same for block range r of R: stream j's blocks [blocks * r / R, blocks * (r + 1) / R), resuming at the bit offset range
 * r - 1 left in d_res (ranges are launched in order on one stream; njobs <= ACM_PARSE_RANGE_MAX_STREAMS) */
#define ACM_PARSE_RANGE_MAX_STREAMS 32768
int acmk_launch_parse_range(const AcmParseJob *d_jobs, uint32_t njobs, const uint8_t *d_files, uint32_t *d_colpos, int16_t *d_idx,
			    acmhip_blkhdr *d_hdr, AcmParseResult *d_res, uint32_t *d_flags, uint64_t max_columns, uint32_t r, uint32_t R,
			    uint32_t stripes_up, acm_block_mark *d_marks, uint32_t parse_slice, uint32_t parse_grid_x, void *stream);
/* the same with byte-plane staging for the jobs that ask for it (mf_rows != 0): d_mf = the byte-plane arena, d_pairs = its pair table,
 * d_blkoff = one word per block (indexed like d_hdr): where the row pair that holds the block's first row starts in its stream's region, in
 * 64-byte units (blocks of an odd height: every other one begins inside a pair).  Streams are walked
 * by the wave-per-stream kernel only (njobs <= ACM_PARSE_RANGE_MAX_STREAMS) */
int acmk_launch_parse_range_mf(const AcmParseJob *d_jobs, uint32_t njobs, const uint8_t *d_files, uint32_t *d_colpos, int16_t *d_idx,
			       acmhip_blkhdr *d_hdr, AcmParseResult *d_res, uint32_t *d_flags, uint64_t max_columns, uint32_t r, uint32_t R,
			       uint32_t stripes_up, uint8_t *d_mf, uint32_t *d_pairs, uint32_t *d_blkoff, acm_block_mark *d_marks, uint32_t parse_slice,
			       uint32_t parse_grid_x, void *stream);
/* Indexed input: njobs jobs (here: windows into streams; a job's file is the byte span of its blocks, data_start unused) whose blocks are
 * the nblock walks of d_bjobs, one wavefront each; then the column kernel over every job, in one piece, int16 rows only.  d_res and d_flags
 * [njobs] must be zero on entry; afterwards job j is clean iff d_res[j].status == 0 && d_res[j].blocks_done == its blocks && d_flags[j] == 0
 * (a walk that fails - data running out, a bad code, a header or an end that disagrees with the index - raises status) */
int acmk_launch_parse_blocks(const AcmParseJob *d_jobs, uint32_t njobs, const AcmBlockJob *d_bjobs, uint32_t nblock, const uint8_t *d_files,
			     uint32_t *d_colpos, int16_t *d_idx, acmhip_blkhdr *d_hdr, AcmParseResult *d_res, uint32_t *d_flags,
			     uint64_t max_columns, uint32_t parse_slice, uint32_t parse_grid_x, void *stream);
/* The block index of njobs streams (<= ACM_PARSE_RANGE_MAX_STREAMS), one wavefront each (acm_index_scan_wave): of a job only file_off, file_len,
 * data_start, level, rows, blocks and hdr_off - here the stream's first entry of d_marks - are read.  Block b of stream j leaves
 * d_marks[hdr_off + b] = { bit, val, pwr }, a walk that covers all its blocks also d_marks[hdr_off + blocks] = { end bit, 0, 0 }; d_res[j] =
 * { blocks done, status, end bit }.  status != 0: data ran out, an invalid filler code, or a ternary symbol out of range (codes 19, 22, 29:
 * validated here, not only skipped) - the exact host reader takes the stream.  Nothing per column is written. */
int acmk_launch_index(const AcmParseJob *d_jobs, uint32_t njobs, const uint8_t *d_files, acm_block_mark *d_marks, AcmParseResult *d_res,
		      void *stream);
/* Striped upload of a block-range batch: every file's arena slot (the file padded to 16 bytes + 16 zero bytes) is cut into R
 * stripes at acmk_stripe_bound(len, s, R); stripe s of all files travels as ONE transfer into a staging arena and a scatter
 * kernel puts the pieces in place, so the first ranges are walked, synthesised and read back while the later stripes are
 * still on their way up (PCIe runs both directions at once).  stripes_up (0 = the whole file is there) tells the walk of a
 * range how many stripes it may read: a stream that needs more stops with a status and goes to the host reader. */
uint32_t acmk_stripe_bound(uint32_t file_len, uint32_t s, uint32_t S);
/* first block of block range r of R (r == R: the end) of a stream of `blocks` blocks whose ranges are cut at multiples of `unit` blocks */
uint32_t acmk_range_bound(uint32_t blocks, uint32_t r, uint32_t R, uint32_t unit);
int acmk_launch_scatter_stripe(const AcmParseJob *d_jobs, uint32_t njobs, const uint64_t *d_stripe_at, const uint8_t *d_stage,
			       uint8_t *d_files, uint32_t s, uint32_t S, void *stream);
int acmk_launch_small(uint32_t level, const AcmDevStream *d_streams, const uint32_t *d_list, uint32_t nlist, uint64_t max_emit,
		      const int16_t *d_idx, const acmhip_blkhdr *d_hdr, int16_t *d_pcm, unsigned fmt, uint32_t list_slice, uint32_t small_grid_x, void *stream);
int acmk_launch_emit(const AcmDevStream *d_streams, const uint32_t *d_list, uint32_t nlist, uint64_t max_emit,
		     const int32_t *d_x, int16_t *d_pcm, unsigned fmt, uint32_t list_slice, void *stream);
/* the float32 builds (acm_kernels_f32.hip), reached through fmt | ACMK_FMT_F32 of the launchers above */
int acmk_launch_fused_f32(uint32_t level, int variant, int cus, int carry, const AcmDevStream *d_streams, const AcmTile *d_tiles,
			  uint32_t ntiles, const int16_t *d_idx, const acmhip_blkhdr *d_hdr, int16_t *d_pcm, unsigned fmt, void *stream);
int acmk_launch_tile2_f32(uint32_t level, int cus, const AcmTile2 *d_tiles, uint32_t ntiles, const int16_t *d_idx, const acmhip_blkhdr *d_hdr,
			  int16_t *d_pcm, int16_t *d_sink, unsigned fmt, void *stream);
int acmk_launch_tile2m_f32(uint32_t level, int cus, const AcmTile2 *d_tiles, uint32_t ntiles, const uint8_t *d_mform, const acmhip_mform_pair *d_pairs,
			   const acmhip_blkhdr *d_hdr, int16_t *d_pcm, int16_t *d_sink, unsigned fmt, uint32_t *d_claim, void *stream);
int acmk_launch_fused_plane_f32(int cus, int carry, const AcmDevStream *d_streams, const AcmTile *d_tiles, uint32_t ntiles,
				const int32_t *d_plane, int16_t *d_pcm, unsigned fmt, void *stream);
int acmk_launch_small_f32(uint32_t level, const AcmDevStream *d_streams, const uint32_t *d_list, uint32_t nlist, uint64_t max_emit,
			  const int16_t *d_idx, const acmhip_blkhdr *d_hdr, int16_t *d_pcm, unsigned fmt, uint32_t list_slice, uint32_t small_grid_x, void *stream);
int acmk_launch_emit_f32(const AcmDevStream *d_streams, const uint32_t *d_list, uint32_t nlist, uint64_t max_emit,
			 const int32_t *d_x, int16_t *d_pcm, unsigned fmt, uint32_t list_slice, void *stream);
/* The dense launchers.  All of them: units, work items, the capped grid and the two refusals (hipErrorInvalidValue for a sub-row of
 * more than 2^31 - 1 units or work past 2^64; nothing to do returns 0) are acm_dense_geo.h's; the four gather kernels share one body
 * (acm_dense_gather.h), and which of them a call launches is acm_dense_tables' answer (acm_dense_layout.h).
 * acm_dense.hip: nrows rows of frames * channels samples each into d_out (int16, or float32 = the int16 sample times 2^-15 with f32), row k at
 * element k * frames * channels: d_rows[k].count samples from d_src + d_rows[k].src, interleaved as they are or (planar, channels == 2) split
 * into a plane per channel, zeros behind them.  d_src: 16-byte aligned; the kernel loads whole aligned 16-byte lines and only lines that hold
 * at least one of a row's samples.  d_out: aligned to its element.  One launch, nothing allocated, nothing waited for */
int acmk_launch_dense_rows(const int16_t *d_src, const AcmDenseRow *d_rows, uint64_t nrows, void *d_out, uint64_t frames, uint32_t channels,
			   int planar, int f32, uint32_t dense_grid, void *stream);
/* acm_dense_mix.hip: the same launch for a row table in which some row carries a converting mode (AcmDenseMode) - the one the
 * batch's layout allows: DOWN with channels == 1, UP_INTER with channels == 2, UP_PLANAR with channels == 2 and planar.  Rows without
 * mode bits are written as acmk_launch_dense_rows writes them.  The same demands on d_src and d_out; a converting row's samples lie
 * inside its slot too */
int acmk_launch_dense_mixed(const int16_t *d_src, const AcmDenseRow *d_rows, uint64_t nrows, void *d_out, uint64_t frames, uint32_t channels,
			    int planar, int f32, uint32_t dense_grid, void *stream);
/* acm_dense_resample.hip: the same launch for a call in which some row is resampled (d_rs[k].L != 0): such a row is filtered from its
 * source samples after their channel conversion; the others are written as acmk_launch_dense_mixed writes them.  d_taps: the tap
 * tables of the call's ratios, 16-byte aligned.  The same demands on d_src and d_out */
int acmk_launch_dense_resample(const int16_t *d_src, const AcmDenseRow *d_rows, const AcmResampleRow *d_rs, const int16_t *d_taps, uint64_t nrows,
			       void *d_out, uint64_t frames, uint32_t channels, int planar, int f32, uint32_t dense_grid, void *stream);
/* acm_dense_speed.hip: the same launch for a call in which some row takes the wide filter (d_sp[k].wide != 0); rows with L != 0
 * and wide == 0 are filtered as acmk_launch_dense_resample filters them, the others written as it writes them.  d_taps: the exact
 * and wide tables of the call, 16-byte aligned.  The same demands on d_src and d_out */
int acmk_launch_dense_speed(const int16_t *d_src, const AcmDenseRow *d_rows, const AcmSpeedRow *d_sp, const int16_t *d_taps, uint64_t nrows,
			    void *d_out, uint64_t frames, uint32_t channels, int planar, int f32, uint32_t dense_grid, void *stream);
/* acm_dense_overlay.hip, behind a dense launch that wrote source row k to d_src + k * row_len (int16; d_src 16-byte aligned, 8 samples
 * of memory behind the last row).  The energy launch adds the sum of squares of every row d_marked names (each once) to
 * d_energy[that row], which the caller has zeroed: one 64-bit atomic add per workgroup, of integers, so the sums do not depend on the
 * order of arrival.  The combine call writes d_res[r] - the gain of every row, from the energies, by a small launch of its own - and
 * then nrows rows of row_len samples to d_out (int16, or float32 = the int16 result times 2^-15 with f32), row r at element
 * r * row_len, by include/acm_hip.h's formula.  Both calls: nothing allocated, nothing waited for; the same kind of loads as
 * acmk_launch_dense_rows */
int acmk_launch_dense_energy(const int16_t *d_src, const uint32_t *d_marked, uint64_t nmarked, uint64_t row_len, uint64_t *d_energy, uint32_t dense_grid,
			     void *stream);
int acmk_launch_dense_overlay(const int16_t *d_src, const AcmOverlayRow *d_rows, const uint64_t *d_energy, AcmOverlayResult *d_res, uint64_t nrows,
			      void *d_out, uint64_t row_len, int f32, uint32_t dense_grid, void *stream);
/* acm_dense_fir.hip, between the two: rows d_rows[i].dst of d_src written from rows d_rows[i].src (other rows, so nothing is read that
 * the launch writes), every channel of frames samples filtered by the row's response out of d_taps (16-byte aligned).  Reads and
 * writes samples of those rows alone, element by element or as whole aligned lines inside a row.  Nothing allocated, nothing waited for */
int acmk_launch_dense_fir(int16_t *d_src, const AcmFirRow *d_rows, uint64_t nfilt, const uint32_t *d_taps, uint64_t frames, uint32_t channels,
			  int planar, uint32_t dense_grid, void *stream);
/* acm_dense_feat.hip, behind the combine launch of a features call.  acmk_launch_feat_twiddle: the B operand of an n_fft-point DFT,
 * acm_feat_twiddle_bytes(n_fft) bytes at d_twiddle (16-byte aligned), from the n_fft cosines at d_cs.  acmk_launch_dense_feat: the
 * features of nrows rows of `frames` int16 samples at d_rows into d_out, float32, nrows * n_mels * F elements in the layout the
 * bank's flags name; reads samples of those rows alone, element by element, and writes those elements alone.  Nothing allocated,
 * nothing waited for */
int acmk_launch_feat_twiddle(const int16_t *d_cs, uint32_t n_fft, void *d_twiddle, void *stream);
int acmk_launch_dense_feat(const int16_t *d_rows, uint64_t nrows, uint64_t frames, const struct AcmFeatDesc *desc, float *d_out, uint32_t dense_grid,
			   void *stream);
/* acmk_launch_dense_logmel: the same with the output line of acm_batch_decode_windows_logmel, by desc's log fields (checked by the
 * caller: acm_feat_log_check).  Without ACM_FEAT_LOG_TOP one launch; with it desc->rowmax is reset on the stream, the feature launch
 * writes L and the rows' maxima, and acmk_launch_feat_log_finish - elements [0, total) of d_out in place, element i of row i / per_row
 * - makes the floats.  Writes those elements and that table alone */
int acmk_launch_dense_logmel(const int16_t *d_rows, uint64_t nrows, uint64_t frames, const struct AcmFeatDesc *desc, float *d_out, uint32_t dense_grid,
			     void *stream);
int acmk_launch_feat_log_finish(float *d_out, uint64_t total, uint64_t per_row, const struct AcmFeatDesc *desc, uint32_t dense_grid, void *stream);
#ifdef __cplusplus
}
#endif

#endif
