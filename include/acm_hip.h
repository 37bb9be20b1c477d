/*
 * acm_hip.h - C ABI of the MI355X-native ACM block-synthesis hot path.
 *
 * This is the boundary a maintainer of the reference would bind to replace the
 * data-parallel half of decode_block()/acm_read() (INTEGRATION.md shows the
 * patch).  Plain C: pointers, sizes, PODs; no C++ or torch types.  Every entry
 * point names the reference code it replaces (paths relative to
 * /root/reference/src).
 *
 * Division of labour (BASELINE.json north_star):
 *   host   - sequential bitstream reader + the 15 filler parsers
 *            (decode.c:41-163, 181-502) -> "staged" form: one int16 filler
 *            index per sample in PCM order + one acmhip_blkhdr per block.
 *   device - amplitude-table unpack (decode.c:592-600 + set_pos :174-177, i.e.
 *            value = idx * val), juggle_block subband synthesis (:508-577) and
 *            16-bit write-out (:617-677) as HIP kernels on gfx950.
 *
 * There is no CPU implementation of the device half in this library; every
 * call fails with ACMHIP_ERR_NO_DEVICE when no HIP device is usable.
 */
#ifndef ACM_HIP_H
#define ACM_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "acm_launch_caps.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ACMHIP_OK             0
#define ACMHIP_ERR_NO_DEVICE -101   /* no usable HIP device / runtime */
#define ACMHIP_ERR_HIP       -102   /* a HIP call failed; see acmhip_last_error() */
#define ACMHIP_ERR_ARG       -103   /* invalid argument */
#define ACMHIP_ERR_NOMEM     -104
#define ACMHIP_ERR_RANGE     -105   /* (rounds 5 / 6: an index a staged form could not hold, acmhip_mform_rows.  Every form holds the whole int16 range now;
                                       the code is kept for callers that test for it and is no longer returned) */

/* output sample layouts = the four writers of decode.c:617-655 */
#define ACMHIP_FMT_S16LE 0u
#define ACMHIP_FMT_S16BE 1u         /* bit 0: big-endian   (bigendianp, decode.c:662) */
#define ACMHIP_FMT_U16LE 2u         /* bit 1: unsigned     (!sgned,     decode.c:663) */
#define ACMHIP_FMT_U16BE 3u

/*
 * Staged block header: the (pwr,val) pair of decode.c:586-589.  On the device
 * the amplitude table midbuf[i] = i*val (decode.c:592-600) is never built;
 * value = (int32)((uint32)idx * val).  pwr is kept for the host (range check
 * of hazard H1) and for diagnostics.
 */
typedef struct acmhip_blkhdr {
	uint32_t val;            /* 0..65535 */
	uint32_t pwr;            /* 0..15 */
} acmhip_blkhdr;

/*
 * Hazard H1: a filler index outside [-2^pwr, 2^pwr) makes the
 * reference read an amplitude-table entry left behind by an EARLIER block
 * (decode.c:809-810: the table is never cleared).  The host parser resolves
 * those samples itself and ships them as patches: "sample `sample` of this
 * stream's staged array has the unpacked value `value`, whatever idx*val says".
 */
typedef struct acmhip_patch {
	uint64_t sample;         /* index into the stream's staged samples (0 = first staged sample) */
	int32_t  value;
	uint32_t stream;         /* index into the acmhip_stream_desc array */
} acmhip_patch;

/*
 * One stream (or one window of a stream) to synthesise.  The staged samples of
 * a stream are contiguous in PCM order: sample m = row*cols + col, rows
 * running on across block boundaries (block b owns rows [b*rows, (b+1)*rows)).
 * The synthesis history of decode.c:803-812 (wrapbuf) is not stored anywhere:
 * it is a pure function of the two staged rows that precede a row
 * (SURVEY.md 7.1), so a window that starts at row_begin > 0 only needs the
 * staged rows row_begin-2.. to be present.  Rows before row 0 are zeros
 * (decode.c:812, util.c:241).
 */
typedef struct acmhip_stream_desc {
	uint64_t idx_off;        /* int16 units from d_idx to staged row 0; multiple of 8 */
	uint64_t hdr_off;        /* acmhip_blkhdr units from d_hdr to the header of block 0.  Header indices are 32 bits wide in the launch
				  * tables: hdr_off + the stream's blocks (ceil(nrows / rows)) <= 2^32, or plan creation returns ACMHIP_ERR_ARG */
	uint64_t pcm_off;        /* int16 units from d_pcm to where sample (row_begin, 0) goes; multiple of 8 */
	uint64_t n_emit;         /* samples to write, starting at row_begin*cols (<= (nrows-row_begin)*cols) */
	uint32_t level;          /* acm_level 0..15 */
	uint32_t rows;           /* acm_rows  1..4095 */
	uint32_t nrows;          /* staged rows present = staged blocks * rows */
	uint32_t row_begin;      /* first row to emit */
} acmhip_stream_desc;

typedef struct acmhip_device acmhip_device;   /* one HIP device + the stream work is queued on */
typedef struct acmhip_plan acmhip_plan;       /* device-resident launch tables for a fixed set of stream descs */

/* which kernel family a plan may use */
#define ACMHIP_PLAN_AUTO      0u    /* one-launch kernels where they apply (levels 0-12 without H1 patches), stage-wise kernels elsewhere */
#define ACMHIP_PLAN_STAGEWISE 1u    /* force the generic stage-wise kernels (bring-up / cross-check) */
/* modifiers (or-ed in) */
#define ACMHIP_PLAN_FORM_ONLY    0x100u  /* streams that come with a byte-plane form are never launched without it: their records over the
                                          * int16 rows are not cut (half the table bytes); a launch with no form bound fails */
#define ACMHIP_PLAN_LEAN_ALWAYS  0x400u  /* whole tiles go to the lean kernels (acm_tile2 / acm_chunk) however few they are - by default a level's
                                          * tiles must fill the chip a few times over to be worth the lean kernels' lead-in tiles.  Small plans
                                          * that want the byte-plane / packed forms read; tests */
#define ACMHIP_PLAN_NO_LEAN      0x800u  /* never the lean kernels: everything on acm_fused_tile / the stage-wise kernels (cross-checks) */
#define ACMHIP_PLAN_FORCE_HALO   0x1000u /* acm_fused_tile: every tile recomputes its two halo rows (default: by tile count) */
#define ACMHIP_PLAN_FORCE_CARRY  0x2000u /* acm_fused_tile: histories carried from tile to tile through LDS (default: by tile count) */
#define ACMHIP_PLAN_UPLOAD_ASYNC 0x200u  /* acmhip_plan_create* returns with the table uploads queued, not done: every launch of the plan
                                          * waits for them on the device (an event wait: do not capture such a launch into a graph) */

const char *acmhip_last_error(void);          /* thread-local text of the last failure */
int  acmhip_device_count(void);               /* usable HIP devices, 0 if none (never fails) */

/* hip_stream: a hipStream_t to queue on (e.g. the caller's framework stream), or NULL for a private one */
int  acmhip_device_open(int ordinal, void *hip_stream, acmhip_device **out);
void acmhip_device_close(acmhip_device *dev);
int  acmhip_device_sync(acmhip_device *dev);
void *acmhip_device_stream(acmhip_device *dev);   /* the hipStream_t in use */

/* memory plumbing so that plain C programs need no HIP headers */
int  acmhip_malloc(acmhip_device *dev, size_t bytes, void **dptr);
int  acmhip_free(acmhip_device *dev, void *dptr);
int  acmhip_host_alloc(size_t bytes, void **hptr);            /* pinned */
int  acmhip_host_free(void *hptr);
int  acmhip_upload(acmhip_device *dev, void *dptr, const void *hptr, size_t bytes);    /* async on the device stream */
int  acmhip_download(acmhip_device *dev, void *hptr, const void *dptr, size_t bytes);  /* async on the device stream */
int  acmhip_memset(acmhip_device *dev, void *dptr, int byte, size_t bytes);            /* async on the device stream: a caller that wants to
                                                                                         * see every sample written (tests, bench) poisons the PCM arena first */

/*
 * Host synthesis (csrc/acm_host_synth.cpp): the SAME contract as a plan over one stream descriptor, on host pointers, without a device -
 * value = idx * val, the cascade of decode.c:508-577, the four writers of :617-655, bit-exact.  It is what acm_read() (include/libacm.h)
 * runs on a box without a usable HIP device, and for streams shorter than acmhip_host_synth_limit() samples while no device handle is
 * open in the process (bringing the HIP runtime up costs more than such a stream's whole decode).  The plan and batch calls never use it.
 * limit: default 128 Msamples (2^27) - measured, not guessed: through acmtool -d on an MI355X box a 41-Msample stream takes 0.16 s on the
 * host path (a few threads over independent tiles), 0.37 - 0.43 s through the GPU (the runtime comes up, the window crosses PCIe twice)
 * and 0.27 s in the reference; at 164 Msamples the two paths meet (0.56 s; the reference: 1.0 s).  0 = the host path only where no device exists; UINT64_MAX = never the device from acm_read().
 */
int  acmhip_host_synth(const acmhip_stream_desc *stream, const int16_t *idx, const acmhip_blkhdr *hdr,
		       const acmhip_patch *patches, size_t npatches, unsigned fmt, int16_t *pcm);
/* The same into float32 samples (see acmhip_plan_launch_f32 for their meaning; pcm_off and n_emit count floats): the CPU reference of
 * the float32 output.  acm_read() never uses it. */
int  acmhip_host_synth_f32(const acmhip_stream_desc *stream, const int16_t *idx, const acmhip_blkhdr *hdr,
			   const acmhip_patch *patches, size_t npatches, float *pcm);
void acmhip_set_host_synth_limit(uint64_t samples);
/* acm_seek_pcm() re-enters a stream at the block in front of its target through the block index the parser keeps (default); off = the
 * reference's way, re-parsing from the first block (util.c:219-242).  Same positions, same PCM; for cross-checks and measurements. */
void acmhip_set_seek_index(int on);
uint64_t acmhip_host_synth_limit(void);

/*
 * Build the launch tables for `n` streams (+ optional H1 patches).  Streams may
 * mix levels/rows/lengths freely.  Replaces nothing in the reference (it has
 * no batching); it is what lets one launch cover thousands of decode_block()s.
 */
int  acmhip_plan_create(acmhip_device *dev, const acmhip_stream_desc *streams, size_t n,
			const acmhip_patch *patches, size_t npatches, unsigned flags,
			acmhip_plan **out);
void acmhip_plan_destroy(acmhip_plan *plan);

/*
 * THE hot path.  Queues unpack + juggle_block + write-out for every stream of
 * the plan: replaces decode.c:592-600 (table), :174-177 (lookup), :528-577
 * (juggle_block), :657-677 (output_values).  d_idx / d_hdr / d_pcm are device
 * pointers; fmt is ACMHIP_FMT_*.  Asynchronous on the device's stream.
 * The launches of one plan follow each other there, and they must: the plan owns small device state that a launch uses and
 * hands on as it found it (the word in which the chunk kernel's wavefronts count the runs of the chunk table they claim - one per
 * level group, zero between launches).  A launch captured into a graph may be replayed any number of times, one replay behind
 * the other; two replays, or a replay and a launch, that could run at the same time need a plan each.
 */
int  acmhip_plan_launch(acmhip_plan *plan, const int16_t *d_idx, const acmhip_blkhdr *d_hdr,
			int16_t *d_pcm, unsigned fmt);

/*
 * The same launch writing float32 samples for torch-style consumers, chosen per launch like fmt.  A float sample is EXACTLY
 * the ACMHIP_FMT_S16LE sample times 2^-15: the reference's own 16-bit value, with its wrap (decode.c:620: the low 16 bits of
 * x >> level, no clamping), divided by 32768 - in [-1, 1), little-endian IEEE, always exact; not a decode at higher precision.
 * pcm_off and n_emit of the stream descriptors count floats (pcm_off stays a multiple of 8: 32 bytes).  Works on any plan except
 * one with a packed arena bound (acmhip_plan_bind_packed): ACMHIP_ERR_ARG, the packed form has no float32 build.
 */
int  acmhip_plan_launch_f32(acmhip_plan *plan, const int16_t *d_idx, const acmhip_blkhdr *d_hdr, float *d_pcm);

/* ------------------------------------------------------------------------
 * Packed staged form: filler class per column pair + fixed-width packed residuals
 * (BASELINE.json north_star: "per-block filler indices plus packed residuals").
 *
 * What set_pos() would store (decode.c:174-177) is an index whose range the column's filler fixes: 0 for the zero filler,
 * |idx| <= 5 for every k / t filler, `ind` bits for a linear one (decode.c:181-476).  Instead of one int16 per sample the
 * host stager ships, for the whole tiles of a stream (acmhip_packed_tile_rows(level) rows x cols, the unit the lean tile
 * kernel works on), per GROUP of rows (acmhip_packed_group_rows) and per PAIR of adjacent columns a width class - 0, 4, 8
 * or 16 bits per index, the narrowest that holds every index of the pair in those rows - and the indices at that width.
 * Column pairs of one class are stored together, so that a wavefront of the kernel unpacks with one code path:
 *
 *   tile  -> acmhip_packed_slots(level) consecutive chunk descriptors, wave-major: the kernel's wave
 *            w owns entries [w * S, (w + 1) * S) of them (S = slots / waves); unused entries have kind 0;
 *   chunk -> 64 UNITS of one group and one class: 64 / NQ column pairs x NQ row quads (NQ = group rows / 4), a unit being
 *            2 columns x the 4 rows row0 + q, row0 + q + NQ, row0 + q + 2 NQ, row0 + q + 3 NQ of its group.  Its blob, at
 *            blob_off16 * 16 bytes: 64 / NQ uint16 (entries >= count unused) that name the column pairs by where their
 *            first column sits in the kernel's padded LDS row (dwords: 2 p + p / 16), then the units, pair-major (pair r,
 *            quad q at index r * NQ + q): kind 4: four dwords, dword k = the unit's k-th row, (int16) column 2p |
 *            (int16) column 2p + 1 << 16;  kind 3: two dwords of int8 (row 0, col 2p), (row 0, 2p + 1), (row 1, 2p),
 *            (row 1, 2p + 1) | rows 2, 3;  kind 2: one dword of eight int4 in the same order;  kind 1: nothing (all zeros).
 *
 * The int16 form stays what every other kernel reads (ragged tails, windows, streams with H1 patches, levels the lean
 * kernel does not take), and what a plan falls back to while no packed arenas are bound.
 * ---------------------------------------------------------------------- */
typedef struct acmhip_packed_chunk {
	uint32_t blob_off16;     /* 16-byte units from the blob arena's base */
	uint16_t count;          /* column pairs in this chunk, 1 .. 64 / NQ */
	uint8_t  kind;           /* ACMHIP_PK_*; 0 = unused entry */
	uint8_t  row0;           /* first row of the chunk's group inside its tile */
} acmhip_packed_chunk;
#define ACMHIP_PK_ZERO   1u
#define ACMHIP_PK_NIBBLE 2u
#define ACMHIP_PK_BYTE   3u
#define ACMHIP_PK_WORD   4u

/* beside acmhip_stream_desc i: rows [0, ntiles * tile_rows) of the stream are staged in packed form as well */
typedef struct acmhip_packed_stream {
	uint64_t chunk_off;      /* ACMHIP_FORM_PACKED: the chunk-table entry the stream's first tile starts at (tile k: chunk_off + k * slots
				  * of its level);  ACMHIP_FORM_BYTEPLANE: the pair-table entry of the pair of zeros in front of the stream
				  * (acmhip_mform_rows).  The packed chunk table is indexed in 64 bits (its records' blob_off16: a blob
				  * below 64 GB).  The byte-plane kernels index the pair table in 32 bits: chunk_off + the stream's entries
				  * (ntiles * acmhip_mform_tile_rows(level) / 2 + 1) + the table's 32 entries of read slack
				  * (acmhip_plan_bind_mform) <= 2^32, or plan creation returns ACMHIP_ERR_ARG; an entry reaches 64 GB of
				  * byte-plane arena (30 bits of 64-byte units) */
	uint32_t ntiles;         /* 0: this stream has no second staged form */
	uint32_t form;           /* ACMHIP_FORM_* */
} acmhip_packed_stream;
#define ACMHIP_FORM_PACKED    0u
#define ACMHIP_FORM_BYTEPLANE 1u

int  acmhip_packed_tile_rows(uint32_t level);     /* rows per packed tile, 0 if the level has no packed form */
int  acmhip_packed_group_rows(uint32_t level);    /* rows that share one width class per column pair */
int  acmhip_packed_slots(uint32_t level);         /* chunk descriptors per tile */
/* upper bound of the blob bytes `ntiles` tiles of `level` can take (incl. the slack the kernel may read past the last unit) */
int  acmhip_pack_bound(uint32_t level, uint64_t ntiles, uint64_t *max_blob_bytes);
/*
 * Host stager, packed half (no device involved): packs `ntiles` consecutive tiles of ONE stream from staged indices
 * idx[row * cols + col] (as acm_stage_file writes them; row 0 = the first row of the first tile) into
 * chunks[0 .. ntiles * slots) and blob[0 .. *blob_bytes).  blob_base: where blob[0] will sit in the batch's blob arena
 * (bytes, multiple of 16); the offsets written are absolute.  Replaces nothing in the reference by itself: it is the
 * storage side of set_pos (decode.c:174-177).
 */
int  acmhip_pack_tiles(uint32_t level, const int16_t *idx, uint64_t ntiles, acmhip_packed_chunk *chunks, uint8_t *blob,
		       uint64_t blob_base, uint64_t *blob_bytes);
/* the inverse, for tests and tools: one tile's descriptors -> idx[tile_rows * cols] (blob = the arena's base) */
int  acmhip_unpack_tile(uint32_t level, const acmhip_packed_chunk *tile_chunks, const uint8_t *blob, int16_t *idx);

/* acmhip_plan_create with the packed form of (some of) the streams: packed[i].ntiles whole tiles of stream i, from its
 * row 0 on, go to the packed build of the lean tile kernel once arenas are bound.  packed may be NULL. */
int  acmhip_plan_create_packed(acmhip_device *dev, const acmhip_stream_desc *streams, size_t n, const acmhip_packed_stream *packed,
			       const acmhip_patch *patches, size_t npatches, unsigned flags, acmhip_plan **out);
/* device tables the packed tiles of this plan are read from by every later launch (both NULL: back to the int16 form) */
int  acmhip_plan_bind_packed(acmhip_plan *plan, const acmhip_packed_chunk *d_chunks, const uint8_t *d_blob);

/* ------------------------------------------------------------------------
 * Byte-plane staged form: the staged indices in the order the matrix cores take them, every row pair at the narrowest
 * width class that holds it.
 *
 * The first stages of the cascade (decode.c:527-590) are linear; over one residue class of the columns (columns
 * c + q * cols/G, q < G, G = acmhip_mform_group(level)) the first log2(G) of them are one banded integer matrix over
 * rows, and a level that has such a build (acmhip_mform_tile_rows(level) != 0: levels 7-14) runs it on
 * v_mfma_i32_16x16x32_i8 / 16x16x64_i8 instead of the vector ALU: its operands are the staged indices themselves (the
 * multiply by the block's val moves behind the matrix), as signed bytes.  A block's indices lie in [-2^pwr, 2^pwr)
 * (decode.c:592-600: the amplitude table has 2^(pwr+1) entries), so quiet blocks need fewer bits.
 *
 *   stream -> a pair of zero rows (what the cascade sees in front of row 0), then its row pairs (rows 2P, 2P + 1), each at
 *             its own width class, back to back (a pair takes 64 bytes or a multiple); acmhip_mform_pair k of the stream =
 *             where pair k - 1 starts (64-byte units from the arena's base) << 2 | class code;
 *   pair   -> its two rows, each row = cols/G residues c, each residue = the G indices of columns c, c + cols/G, ...
 *
 * G = 64, levels 8-14 (six stages on the matrix cores: acm_chunk at levels 8-12, acm_tile2 at 13 / 14).  The pair in front is
 * at 8 bits.  Per residue:
 *             ACMHIP_BP_BYTE  (2)  64 bytes: idx itself (every index of the pair in [-128, 127])
 *             ACMHIP_BP_NIB12 (1)  levels 8-12 only: idx = 256 hi + lo with lo a signed byte and hi a signed NIBBLE (every index of
 *                                  the pair in [-2176, 1919]): 64 low bytes, then 32 bytes of high nibbles in the order the kernel's
 *                                  lanes read them - lane ks < 4 (columns q = 16 ks .. 16 ks + 15 of the class) takes the 8 bytes
 *                                  at 64 + 8 ks: dword d < 2 holds its elements 8 d .. 8 d + 7, element 8 d + b (b < 4) in the HIGH
 *                                  nibble of byte b, element 8 d + 4 + b in the low one (x & 0xf0f0f0f0 and (x << 4) & 0xf0f0f0f0
 *                                  are then the matrix operand bytes hi << 4 of elements 8 d .. + 3 and 8 d + 4 .. + 7)
 *             ACMHIP_BP_WORD  (3)  idx = 256 hi + lo with BOTH bytes signed: 64 low bytes, then 64 high bytes.  That ends at
 *                                  32 639; a pair with a larger index (it takes pwr 15) is written as
 *             ACMHIP_BP_WORDU (0)  idx = 256 hi + lo with hi = idx >> 8 (signed) and lo the UNSIGNED low byte,
 *                                  stored minus 128 ((idx & 0xff) ^ 0x80: a signed byte for the matrix instruction; the kernels
 *                                  add 128 x val x the coefficient row sums of such rows back): the whole int16 range, same
 *                                  64 + 64 bytes.  (Levels 8-14; no stream is refused for its indices any more)
 * G = 8, level 7 (three stages, acm_tile2; also levels 8-9, and G = 16 at 10-14, in a -DACM_TUNING build run with ACM_K3=0).  The
 * pair in front is at 4 bits.  Per residue:
 *             ACMHIP_BP_WORD    G low bytes ((idx & 0xff) ^ 0x80: signed bytes, the kernel adds the 128 back through the
 *                               accumulator), then G high bytes (idx >> 8)
 *             ACMHIP_BP_BYTE    G bytes (idx itself; every index of the pair in [-128, 127])
 *             ACMHIP_BP_NIBBLE  G / 2 bytes (every index in [-8, 7]): per dword eight indices plus 8 each, index 8 j + i in
 *                               nibble 2 i, index 8 j + 4 + i in nibble 2 i + 1 (i < 4)
 *
 * Only whole tiles are staged this way, the ragged tail of a stream stays int16 (as with the packed form).  Whoever writes the
 * form (acmhip_mform_rows, acm_stage_file_mform, the device parser) and the kernel that reads it are the same library build: the
 * form of a level follows the kernel the build ships for it.
 * ---------------------------------------------------------------------- */
typedef uint32_t acmhip_mform_pair;
#define ACMHIP_BP_WORDU  0u     /* the six-stage form of levels 8-12: 16 bits over the WHOLE int16 range (see above) */
#define ACMHIP_BP_NIBBLE 1u
#define ACMHIP_BP_NIB12  1u     /* the same code in the six-stage form of levels 8-12 (which has no 4-bit class): 12 bits, see above */
#define ACMHIP_BP_BYTE   2u
#define ACMHIP_BP_WORD   3u
int  acmhip_mform_tile_rows(uint32_t level);     /* rows per tile of the matrix-core build, 0 if the level has none */
int  acmhip_mform_group(uint32_t level);         /* columns of a residue class kept side by side: 64 (levels 8-14, a six-stage first pass), 8 (level 7: three); 0 if none */
uint64_t acmhip_mform_bytes(uint32_t level, uint64_t nrows);     /* upper bound of the bytes nrows rows take (every pair at 16 bits, + the pair in front and 64 bytes of read slack) */
uint64_t acmhip_mform_pairs(uint64_t nrows);                     /* pair-table entries of nrows rows: nrows / 2 + 1 */
/*
 * Host stager, byte-plane half: idx[row * cols + col] (as acm_stage_file writes them; nrows even) -> out[0 .. *bytes_used) and
 * pairs[0 .. nrows / 2].  blob_base: where out[0] will sit in the batch's arena (bytes, multiple of 64, < 64 GB); the
 * offsets written are absolute.
 */
int  acmhip_mform_rows(uint32_t level, const int16_t *idx, uint64_t nrows, uint8_t *out, uint64_t blob_base, acmhip_mform_pair *pairs,
		       uint64_t *bytes_used);
/* the inverse, for tests and tools (blob = the arena's base) */
int  acmhip_mform_unrows(uint32_t level, const uint8_t *blob, const acmhip_mform_pair *pairs, uint64_t nrows, int16_t *idx);
/* device arena and pair table the byte-plane tiles of this plan are read from by every later launch (both NULL: back to the int16 form).
 * The table must be readable 32 entries past its last one (the kernel fetches entries in groups through the scalar cache), the arena
 * 64 bytes past the last pair (acmhip_mform_rows leaves that slack behind every block it writes). */
int  acmhip_plan_bind_mform(acmhip_plan *plan, const uint8_t *d_mform, const acmhip_mform_pair *d_pairs);

/* introspection for benchmarks/tests */
typedef struct acmhip_plan_stats {
	uint64_t samples;        /* total n_emit */
	uint64_t tiles;          /* fused-kernel workgroups */
	uint32_t fused_streams;  /* streams handled by a one-launch kernel (fused tile kernel, levels 5-12; register kernel, levels 0-4) */
	uint32_t stagewise_streams;
	uint32_t launches;       /* kernel launches per acmhip_plan_launch */
	uint32_t reserved;
	uint32_t mform_tiles;    /* tiles of streams that came with a byte-plane form (read from it while an arena is bound: acmhip_plan_bind_mform) */
	uint32_t packed_tiles;   /* tiles that have records of the packed build too (read in packed form while arenas are bound: acmhip_plan_bind_packed) */
} acmhip_plan_stats;
int  acmhip_plan_get_stats(const acmhip_plan *plan, acmhip_plan_stats *out);
/* rows [row_begin, row_begin + *rows) of stream `stream` (its position among the descriptors the plan was created from) are read from the
 * stream's second staged form by this plan's launches while one is bound - every other row it decodes, and the two rows in front of them,
 * from the int16 arena.  (row_begin > 0: a window that starts on a tile boundary of a stream with a byte-plane form - the form must hold
 * the stream's rows from row 0 to the window's last whole tile.)  0 for a stream without a second form, and for one whose form the plan does not use (a level-13 / 14 stream of a small plan, a
 * stage-wise plan): a caller that stages both forms uploads the int16 rows from max(*rows - 2, 0) on. */
int  acmhip_plan_form_rows(const acmhip_plan *plan, size_t stream, uint64_t *rows);

/*
 * Fill mode of a device handle: a debugging aid that only tests turn on (bench.py, acmtool and the measurement scripts never do; there
 * is no environment variable for it).  Off, the default, the library does what it did without it.  The staging arenas of a handle are
 * grow-only and reused by every batch, window and index call, and the device blocks of destroyed plans are handed to the next plan, so
 * a call works at the addresses of the one before it - a kernel that skips a column, a table entry nobody wrote or a read-back that
 * was dropped finds the previous call's bytes, which for a test that decodes the same files again are the right ones.  On:
 *   - every staging arena is filled over exactly the bytes the call asks of it before the call's first use of it, once per call (a
 *     second request for the same arena inside one call fills only what it asks beyond the first): device arenas by a memset that has
 *     ended before the call goes on, pinned ones by memset();
 *   - every device block a plan is given (recycled or new: tile tables, stream lists, the stage-wise planes, the lead-in sink) is
 *     zeroed before the plan's tables are queued.  Blocks of live plans are never touched.
 * The PCM arenas (device and pinned) are filled with 0xA5 bytes - whatever the output type: a float32 call sees 0xA5A5A5A5 words -,
 * the int16 index arenas with 0x5A bytes (the index 0x5A5A: indices are only ever operands), everything else with zeros: file images,
 * job tables, column offsets, pair and chunk tables, byte-plane and packed blobs, block headers and marks are places, classes, offsets
 * and loop bounds, read past what a call wrote by design (acmhip_plan_bind_mform), and zero is a valid one in each.  The mode can make
 * a comparison fail; it cannot make a kernel read from anywhere it could not read from before.
 * Returns the previous state (0 / 1), or ACMHIP_ERR_ARG.  Waits for a batch call that is using the handle.
 */
int  acmhip_device_set_fill(acmhip_device *dev, int on);
/* Staging arena `slot` (0, 1, ... until ACMHIP_ERR_ARG) of the handle, for tests of the above; every out pointer may be NULL.  *name: a
 * static string ("D_IDX", "H_PCM", ...); *ptr: where it is now (NULL: never allocated; device memory unless *is_host: pinned); *bytes:
 * what the last call that held the handle's arenas asked of it (0: that call did not use it); *fill: the byte the fill mode puts there.
 * Not while a call is using the handle. */
int  acmhip_device_arena_info(acmhip_device *dev, int slot, const char **name, void **ptr, size_t *bytes, int *is_host, int *fill);
/*
 * Launch caps: a debugging aid like the fill mode, for tests only.  Some launchers walk a list longer than one grid in slices, and some
 * cap their grid and let the kernel stride over the rest (acm_launch_caps.h names the five limits and the kernels behind them).  At
 * the built-in limits a second slice or a second trip takes 65 536 streams, 32 M samples of one level 0-4 stream or a million dense
 * rows; with a limit lowered, a test of a few streams walks the same path.  A cap can only be lowered: a field of 0 stands for the
 * built-in value, a field above it makes the call return ACMHIP_ERR_ARG with nothing changed.  caps == NULL: the built-in values.
 * *previous (may be NULL): the caps in force before the call, as they were set (0 = built-in).  The handle keeps the caps and hands
 * them to its launchers as plain arguments: there is no process-wide state, other handles are not affected, and a launch still asks
 * nothing of the runtime.  No cap changes a result - only how many launches or trips produce it.  Waits for a batch call that is
 * using the handle; a plan launched while the call runs may see either set.
 */
int  acmhip_device_set_launch_caps(acmhip_device *dev, const acmhip_launch_caps *caps, acmhip_launch_caps *previous);

/*
 * Time `reps` back-to-back acmhip_plan_launch calls with HIP events recorded on
 * the launch stream; *ms_total receives the elapsed milliseconds of the whole
 * bracket (device time, includes launch gaps).  Blocks until done.
 */
int  acmhip_plan_time(acmhip_plan *plan, const int16_t *d_idx, const acmhip_blkhdr *d_hdr,
		      int16_t *d_pcm, unsigned fmt, int reps, float *ms_total);

/* ------------------------------------------------------------------------
 * Host half of the path: bit parsing into staged form.
 * Replaces decode.c:41-163 (bit reader), :181-502 (fillers, fill_block),
 * :586-589 (block header), :687-752 (headers) for in-memory files: whole
 * (acm_stage_file), or a run of blocks entered through a block index
 * (acm_index_file, acm_stage_window).
 * ---------------------------------------------------------------------- */
typedef struct acm_stage_info {
	uint32_t level, rows, cols;
	uint32_t channels;       /* in effect (after force_chans) */
	uint32_t hdr_channels;   /* as written in the header */
	uint32_t rate;
	uint32_t total_values;
	uint32_t wavc;
	uint32_t blocks;         /* blocks completely parsed into the staging arrays */
	int32_t  end_status;     /* 0 = clean end (EOF at a block/column boundary or total_values reached);
	                            ACM_ERR_* = what acm_read would have returned after those blocks */
	uint64_t npatches;       /* H1 patches produced */
	uint64_t header_bytes;   /* 14 or 42 */
} acm_stage_info;

/* header only (decode.c:712-752 + channel forcing :795-798); returns ACM_OK or ACM_ERR_NOT_ACM */
int  acm_stage_probe(const uint8_t *data, size_t len, int force_chans, acm_stage_info *info);

/*
 * Parse every block that acm_read() would decode (stops after the block that
 * covers total_values, at a clean EOF, or at the first error) into
 *   idx[b*block_len + row*cols + col]  (row-major, PCM order) and hdr[b].
 * max_blocks bounds the arrays; patches (may be NULL when max_patches == 0)
 * receive H1 fix-ups with .stream = 0.  Returns ACM_OK (details in *info) or
 * ACM_ERR_NOT_ACM / ACMHIP_ERR_ARG.
 */
int  acm_stage_file(const uint8_t *data, size_t len, int force_chans,
		    int16_t *idx, acmhip_blkhdr *hdr, size_t max_blocks,
		    acmhip_patch *patches, size_t max_patches, acm_stage_info *info);

/*
 * The same, with the whole tiles of the stream written in the byte-plane form as they are parsed (block by block, out of the cache)
 * instead of by a second pass over idx: rows [0, *mf_rows) - whole tiles of the lean kernel - go to mf_out (pairs / mf_base /
 * *mf_bytes as acmhip_mform_rows writes them; room for acmhip_mform_bytes() / acmhip_mform_pairs() of every row the header
 * promises) and idx receives only the rows from *mf_rows - 2 on, which is all the int16 kernels read of such a stream.
 * *mf_rows = 0: the stream has no form (its level - levels 13 / 14 included, whose int16 rows a plan too small for the lean kernel
 * reads from row 0 on -, H1 patches - then info->npatches says so and a caller of this call stages again with room for them (the
 * library's own callers get them from the same pass) -, a file that
 * ends early) and idx holds every row.  Every index has a place in the form (the whole-range class).  Any block height: a row pair
 * may lie across two blocks.
 */
int  acm_stage_file_mform(const uint8_t *data, size_t len, int force_chans, int16_t *idx, acmhip_blkhdr *hdr, size_t max_blocks,
			  acm_stage_info *info, uint8_t *mf_out, uint64_t mf_base, acmhip_mform_pair *pairs, uint64_t *mf_rows,
			  uint64_t *mf_bytes);

/* ------------------------------------------------------------------------
 * Block index (csrc/acm_stage.cpp; no reference counterpart - the reference re-parses a stream from its first block to seek,
 * util.c:219-242).  A block depends on the blocks in front of it in two ways only: where it starts, and what they left in the
 * never-cleared amplitude table (hazard H1), which their (val, pwr) headers determine.  With one mark per block a reader enters
 * the stream at any block and stages exactly what a reader that came from the header would.
 * ---------------------------------------------------------------------- */
typedef struct acm_block_mark {  /* 16 bytes, plain data: callers may write it to disk and read it back */
	uint64_t bit;            /* file bit offset of the block's first bit (its 20-bit header) */
	uint32_t val, pwr;       /* the block's header: all the stale-table history (H1) needs */
} acm_block_mark;

/*
 * Parses like acm_stage_file and stores no indices: marks[b] for every block acm_stage_file would stage, b < info->blocks, and
 * one entry more - marks[info->blocks].bit = the bit behind the last whole block, val = pwr = 0.  marks has room for
 * max_blocks + 1 entries.  *info is what acm_stage_file reports for the same bytes.  No device involved.
 */
int  acm_index_file(const uint8_t *data, size_t len, int force_chans,
		    acm_block_mark *marks, size_t max_blocks, acm_stage_info *info);

/*
 * Host staging of blocks [block_first, block_first + block_count) entered through the index marks[0 .. nblocks_indexed] of this
 * very file: idx, hdr and the patches are that slice of what acm_stage_file writes (patch.sample counted from the first staged
 * sample of block_first; values resolved against the table history of the blocks in front, taken from the marks).
 * info->blocks = blocks staged here, info->end_status = what stopped it (0: block_count reached, or the stream's clean end).
 * The index is checked before use - bits strictly increasing, behind the header, inside the file, block_first <=
 * nblocks_indexed: ACMHIP_ERR_ARG - and while parsing: an indexed block that does not have the header its mark names, does not
 * end where the next mark says or is not whole ends the window with ACM_ERR_CORRUPT.  A wrong index never reads out of bounds.
 * (What nothing in a window can contradict is the (val, pwr) of the marks in FRONT of it: they are only the table history that H1
 * patch values are resolved against.)
 */
int  acm_stage_window(const uint8_t *data, size_t len, int force_chans,
		      const acm_block_mark *marks, size_t nblocks_indexed,
		      uint32_t block_first, uint32_t block_count,
		      int16_t *idx, acmhip_blkhdr *hdr,
		      acmhip_patch *patches, size_t max_patches, acm_stage_info *info);

/* ------------------------------------------------------------------------
 * Batch front end (no reference counterpart; BASELINE.json "batch-of-files").
 * Decodes n in-memory ACM files on ONE device: threaded host staging ->
 * pinned buffers -> H2D -> acmhip_plan_launch -> D2H, pipelined in chunks of
 * whole streams so that the five steps overlap.
 * ---------------------------------------------------------------------- */
typedef struct acm_batch_item {
	const uint8_t *data;     /* in:  file image */
	size_t   len;            /* in */
	int16_t *pcm;            /* in:  caller buffer for total_values words (may be NULL: decode and discard) */
	size_t   pcm_cap;        /* in:  capacity of pcm in 16-bit words */
	uint64_t words;          /* out: words actually decoded (<= total_values) */
	int32_t  status;         /* out: ACM_OK, or the ACM_ERR_* that ended the stream / rejected the file */
	uint32_t level, rows, channels, rate, total_values;   /* out */
	uint32_t reserved;
	uint64_t dev_off;        /* out: 16-bit word offset of this stream's PCM inside opts->d_pcm (device-resident output; float
	                            offset with ACM_BATCH_PCM_F32) */
} acm_batch_item;

typedef struct acm_batch_opts {
	int      force_chans;
	unsigned fmt;            /* ACMHIP_FMT_* */
	int      threads;        /* host staging threads, 0 = hardware concurrency */
	unsigned plan_flags;     /* ACMHIP_PLAN_* */
	unsigned parse;          /* ACM_BATCH_PARSE_* */
	unsigned flags;          /* ACM_BATCH_* below (0: none) */
	void    *d_pcm;          /* NULL: PCM goes to items[i].pcm in host memory.  Otherwise a device buffer of
	                            d_pcm_words 16-bit words (>= acm_batch_pcm_words()): PCM stays in HBM, stream i at
	                            d_pcm + items[i].dev_off, nothing is copied back (items[i].pcm is ignored) */
	uint64_t d_pcm_words;
	const struct acm_batch_prestaged *prestaged;    /* NULL, or what acm_batch_prestage made of these very items: the bit
	                                                   parsing is done already (forces ACM_BATCH_PARSE_HOST semantics) */
} acm_batch_opts;

/* opts->flags */
#define ACM_BATCH_STAGE_PACKED 2u   /* host parsing only: the pool also packs the whole tiles of every clean stream (acmhip_pack_tiles) and the
                                       upload carries the packed form + the int16 rows the other kernels still read (ragged tails) instead
                                       of the whole int16 arena - about half the bytes over PCIe and through HBM, for ~30 % more host
                                       work per stream and a synthesis launch that is 10-18 % slower (acm_tile2p).  Off by default. */
#define ACM_BATCH_STAGE_BYTEPLANE 4u /* the default, spelled out: whoever parses the bits - the host pool (acm_stage_file_mform) or the device parser's
                                       column kernel - writes the whole tiles of every clean stream of levels 7-14 in the byte-plane form (same bytes as
                                       int16 rows) and only the rows the other kernels still read as int16; the synthesis launch runs its first pass on
                                       the matrix cores (+3 ... +24 % by level).  Wins over ACM_BATCH_STAGE_PACKED when both are set. */
#define ACM_BATCH_STAGE_INT16  8u   /* every row is staged as int16, no second form (the round-1 ... round-4 default; measurements, cross-checks) */
#define ACM_BATCH_RANGES(n)    (((unsigned)(n) & 0xFFu) << 8)  /* device parsing: walk and decode the batch in n block ranges (1 = in one piece;
                                       0 = the library decides: by the length of the longest stream).  Bits 8-15 of opts->flags */
#define ACM_BATCH_PCM_PINNED   1u   /* every items[i].pcm is pinned host memory (acmhip_host_alloc): the read-back engine writes
                                       the PCM straight into it, stream by stream, instead of through the library's own pinned
                                       arena and a host copy (taken for streams of 64 KB of PCM and more on average) */
#define ACM_BATCH_PCM_F32     16u   /* device-resident output only: float32 samples into opts->d_pcm, each the ACMHIP_FMT_S16LE sample
                                       times 2^-15 exactly (acmhip_plan_launch_f32); d_pcm_words and items[i].dev_off count floats
                                       (acm_batch_pcm_words() counts samples: unchanged).  ACMHIP_ERR_ARG without opts->d_pcm, with a
                                       fmt other than ACMHIP_FMT_S16LE, or with ACM_BATCH_STAGE_PACKED */

/* where the bit parsing of a batch runs */
#define ACM_BATCH_PARSE_HOST   0u   /* host thread pool (default; the exact reader, any stream) */
#define ACM_BATCH_PARSE_DEVICE 1u   /* one GPU lane per stream for clean streams; streams the device parser is not
                                       sure about (data running out, corrupt symbols, hazard H1, files >= 256 MiB) are
                                       re-parsed by the host reader.  Pays off for thousands of streams per batch. */
#define ACM_BATCH_PARSE_AUTO   2u   /* DEVICE when the batch is worth at least 5 x threads streams of its longest stream's
                                       size (9 x from 1024 streams, 16 x from 32 K streams on), HOST below that: walking a
                                       stream is sequential, and a wavefront walks 5-16x slower than one host core parses */

typedef struct acm_batch_timing {
	double stage_s;          /* wall clock until the last stream was bit-parsed (headers included, allocation not) */
	double h2d_s, kernel_s, d2h_s;   /* device-side durations summed over the pipeline's chunks; they overlap
	                                    each other and the parsing, so they do not add up to total_s */
	double total_s;          /* wall clock of the whole call */
	uint64_t samples;
	double alloc_s;          /* pinned + device arena allocation */
	uint64_t device_parsed;  /* ACM_BATCH_PARSE_DEVICE: streams staged by the device parser ... */
	uint64_t host_parsed;    /* ... and streams (re)parsed by the host reader */
	uint64_t packed_streams; /* ACM_BATCH_STAGE_PACKED: streams whose whole tiles travelled in packed form */
	uint64_t h2d_bytes;      /* staged bytes (indices in either form, block headers, file images for the device parser) sent to the device */
} acm_batch_timing;

int  acm_batch_decode(acmhip_device *dev, acm_batch_item *items, size_t n,
		      const acm_batch_opts *opts, acm_batch_timing *timing);

/*
 * The host half of acm_batch_decode ahead of time, WITHOUT a device: bit-parses the items' files into staged form
 * (host thread pool, opts->threads / force_chans as above) kept in memory this call allocates.  A later
 * acm_batch_decode on the same items with opts->prestaged = *out copies that into its upload arenas instead of
 * parsing - a front end can parse the next groups of files while the device works on the current one, or while the
 * HIP runtime is still coming up (libacm_amd/csrc/acmtool.c -B).  *seconds (may be NULL): wall clock of the parsing.
 */
typedef struct acm_batch_prestaged acm_batch_prestaged;
int  acm_batch_prestage(const acm_batch_item *items, size_t n, const acm_batch_opts *opts, acm_batch_prestaged **out, double *seconds);
void acm_batch_prestage_free(acm_batch_prestaged *p);

/* Optional, for applications that know they are about to decode through the libacm.h calls (acmtool -d): start opening
 * the process-wide default device - HIP runtime, device handle, the kernels' code object - on a thread of the library's
 * own and return at once.  The first acm_read() that needs the GPU waits for it; until then the stream keeps parsing
 * ahead on the calling thread.  Without this call the device is opened by that first acm_read() itself (a process that
 * only opens, seeks or inspects streams never touches the GPU).  No reference counterpart. */
void acmhip_prewarm(void);

/* 16-bit words of device memory acm_batch_decode needs for the PCM of these files (headers only are read;
 * every stream is padded to a multiple of 64 words) - the size of opts->d_pcm for device-resident output */
uint64_t acm_batch_pcm_words(const acm_batch_item *items, size_t n, int force_chans);

/* ------------------------------------------------------------------------
 * Windowed batch decode (csrc/acm_batch_windows.cpp over the layout of csrc/acm_window_layout.cpp): random-access crops out of
 * many files in one call, at a cost proportional to the windows - bit parsing, PCIe, synthesis and stores - not to the files.
 * Needs the block index of every item.
 *
 * Let `whole` be the items[i].words samples acm_batch_decode delivers for item i.  A window's PCM is
 * whole[first_word : first_word + max_words] clipped to the end of whole, bit for bit; `words` its length (0 for a window that
 * starts behind the end, and for max_words == 0); `status` ACM_OK when the slice has all max_words, else the item's own end
 * status (index[i].end_status: ACM_OK for a stream that simply ended, the parse error of a corrupt or truncated one;
 * ACM_ERR_NOT_ACM for a file that is not ACM, ACMHIP_ERR_ARG for an index the file cannot have).  Windows may overlap, repeat an
 * item and come in any order.
 *
 * A window stages the blocks from the one that holds row max(first_word / cols - 2, 0) - the two rows of synthesis history, see
 * acmhip_stream_desc - to the one that holds its last sample, and is synthesised as a window of that run of blocks which starts
 * with the ROW of its first sample: the up to cols - 1 samples in front of first_word land in the slot in front of dev_off.
 * One plan over int16 rows for all windows of the call.
 *
 * opts: fmt, force_chans, threads, plan_flags, d_pcm / d_pcm_words (>= acm_batch_window_pcm_words()), ACM_BATCH_PCM_F32 (with
 * d_pcm; offsets count floats) as in acm_batch_decode.  prestaged and ACM_BATCH_STAGE_PACKED: ACMHIP_ERR_ARG.  opts->parse:
 *   ACM_BATCH_PARSE_HOST    a thread pool runs acm_stage_window per window into a pinned arena; one upload, one plan, one launch.
 *   ACM_BATCH_PARSE_DEVICE  only the byte span of every window's blocks (from the marks) is uploaded; acm_parse_scan_blocks walks
 *                           every (window, block) as a wavefront of its own - with the index blocks are independent jobs, there is
 *                           no sequential walk of a stream left - and checks the block against its marks, acm_parse_columns
 *                           decodes the columns.  A window the device is not sure about (H1, a bad code, data running out, a block
 *                           that disagrees with its marks, a span of 256 MiB) is staged again by the host; it never fails the call.
 *   ACM_BATCH_PARSE_AUTO    HOST for calls that stage fewer than 256 blocks in all, DEVICE from there on.  Measured on an MI355X with
 *                           16 host threads (profiles/window_decode_notes.txt): the device path costs a second round trip per call
 *                           (the walk's results come back before the plan is cut) and less per block; the two meet between 58
 *                           blocks (16 windows: HOST ahead) and 970 blocks (256 windows: DEVICE ahead).
 * dev == NULL: ACMHIP_ERR_NO_DEVICE.
 * ---------------------------------------------------------------------- */
typedef struct acm_batch_index {         /* one per item */
	const acm_block_mark *marks;     /* blocks + 1 entries, as acm_index_file wrote them (may be NULL for a file that is not ACM) */
	uint32_t blocks;                 /* acm_stage_info.blocks of acm_index_file */
	int32_t  end_status;             /* acm_stage_info.end_status of acm_index_file */
} acm_batch_index;

typedef struct acm_batch_window {
	uint32_t item;           /* in:  which items[] entry */
	uint32_t reserved;       /* in:  read by acm_batch_decode_windows_dense with ACM_DENSE_SPEED alone: the window's speed */
	uint64_t first_word;     /* in:  first interleaved 16-bit sample wanted */
	uint64_t max_words;      /* in */
	int16_t *pcm;            /* in:  host output for min(words, pcm_cap) samples (ignored with opts->d_pcm; may be NULL) */
	size_t   pcm_cap;
	uint64_t words;          /* out */
	int32_t  status;         /* out */
	uint32_t reserved2;
	uint64_t dev_off;        /* out: where the window's FIRST REQUESTED sample is in opts->d_pcm (samples) */
	uint64_t slot_off, slot_words;   /* out: the region of opts->d_pcm the library may have written for this window */
} acm_batch_window;

typedef struct acm_window_timing {
	double stage_s;          /* wall clock until every window was bit-parsed (host pool, or device walk + host re-staging) */
	double h2d_s, kernel_s, d2h_s;   /* device-side durations: uploads, synthesis launch, read-back */
	double total_s;          /* wall clock of the whole call */
	uint64_t samples;        /* samples delivered (sum of words) */
	double alloc_s;          /* pinned + device arena allocation */
	uint64_t device_parsed;  /* windows staged by the device parser ... */
	uint64_t host_parsed;    /* ... and windows (re)staged by the host reader */
	uint64_t h2d_bytes;      /* bytes sent to the device: staged indices and headers, or byte spans and job tables */
	uint64_t blocks_parsed;  /* blocks bit-parsed by anyone, host or device: the sum of the windows' block ranges (+ the ranges the host
	                            staged again) - nothing in front of a window is parsed */
} acm_window_timing;

/* samples of device memory acm_batch_decode_windows needs for these windows at most (headers only are read; every window's slot
 * is padded to a multiple of 64) - the size of opts->d_pcm for device-resident output */
uint64_t acm_batch_window_pcm_words(const acm_batch_item *items, size_t n, const acm_batch_window *wins, size_t nwin, int force_chans);
/* items: data / len are read, nothing is written.  index[i] belongs to items[i]. */
int  acm_batch_decode_windows(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index,
			      acm_batch_window *wins, size_t nwin, const acm_batch_opts *opts, acm_window_timing *timing);

/* ------------------------------------------------------------------------
 * Dense crop batches (csrc/acm_batch_windows.cpp over csrc/acm_dense_layout.cpp, kernel: csrc/acm_dense.hip): the windows of
 * acm_batch_decode_windows as ONE tensor of equally spaced, zero-padded rows - what a training step consumes - instead of slots at
 * arbitrary 2-byte alignments with ragged lengths and interleaved channels.
 *
 * The output is opts->d_pcm (device memory, required): nwin rows of R = frames * channels samples, row k at sample k * R; int16, or
 * float32 with ACM_BATCH_PCM_F32 (the int16 sample times 2^-15 exactly, as acmhip_plan_launch_f32 writes it).  opts->d_pcm_words
 * counts samples of the output type and is at least nwin * R.  With `whole` and `words` as acm_batch_decode_windows defines them,
 * element e of row k is whole[first_word + j] where j < words and zero (int16 0, float +0.0) elsewhere;
 *   interleaved (default)   j = e:                          the row is [frames][channels]
 *   ACM_DENSE_PLANAR        j = (e % frames) * channels + e / frames: the row is [channels][frames]
 * Every element of all nwin rows is written, the rows of windows that deliver nothing included; nothing outside [0, nwin * R) is.
 *
 * wins[k].words and .status are what acm_batch_decode_windows reports for the same window - also for one the host stager turns
 * away during the call (a stale or damaged index): its error status, a row of zeros.  dev_off = slot_off = k * R, slot_words = R.
 * A window whose item has, in effect (after force_chans), another channel count than dense->channels is - without ACM_DENSE_MIX,
 * below - turned away softly, as a file that is not ACM is: words = 0, status = ACMHIP_ERR_ARG, a row of zeros; nothing of it is
 * parsed, uploaded or synthesised (timing->blocks_parsed shows it) and the call does not fail.
 *
 * ACMHIP_ERR_ARG before anything is written: dense == NULL, frames == 0, channels other than 1 or 2, unknown dense->flags;
 * opts->d_pcm == NULL or too small; a fmt other than ACMHIP_FMT_S16LE (padding has no single meaning in the other writers);
 * prestaged or ACM_BATCH_STAGE_PACKED; a window with max_words > R, or with first_word or max_words that is no multiple of
 * channels.  dev == NULL: ACMHIP_ERR_NO_DEVICE.
 *
 * The windows are synthesised as by acm_batch_decode_windows - one plan over int16 rows, float output too - into an arena of the
 * handle's own; nothing is read back.  One launch of acm_dense_rows behind the plan's, on the same stream, reads a row table of 16
 * bytes per window and copies, splits the channels, widens and pads; the call returns with the stream drained.
 * timing->kernel_s covers synthesis and that launch.
 *
 * ACM_DENSE_MIX: mono and stereo files in one batch.  Without the flag nothing of the above changes.  With it, a window whose item
 * has the OTHER channel count c_k (1 or 2, after force_chans) than C = dense->channels is decoded and converted instead of turned
 * away.  Its first_word and max_words count the item's own interleaved samples, as in acm_batch_decode_windows, and so do `whole`
 * and `words`; it delivers f = words / c_k frames, source frame i being whole[first_word + i * c_k + ch], and with T = frames its
 * row holds, for i < f,
 *   c_k == 2, C == 1                     (L_i + R_i) >> 1: the sum in 32 bits, the shift arithmetic - the floor, so 32767 + 32767
 *                                        gives 32767 and -1 + 0 gives -1
 *   c_k == 1, C == 2, interleaved        the sample in both channels: out[2i] = out[2i + 1] = s_i
 *   c_k == 1, C == 2, ACM_DENSE_PLANAR   the sample in both planes:   out[i] = out[T + i] = s_i
 * and zeros in the frames i >= f.  float32 is that int16 result times 2^-15: the down-mix is defined on integers, once.  Every
 * element of every row is written and nothing outside [0, nwin * R), as without the flag.  A window whose item has C channels gets
 * exactly the row it gets without the flag.
 * The checks of such a window count in the item's own frames: first_word % c_k == 0, max_words % c_k == 0 and
 * max_words <= T * c_k, else ACMHIP_ERR_ARG for the whole call before anything is written.  Windows without a channel count - of an
 * item that is not ACM, whose index is unusable, or that does not exist - are checked against C and deliver a row of zeros, as
 * without the flag.  wins[k].words (SOURCE samples) and .status are what acm_batch_decode_windows reports for the same window;
 * dev_off = slot_off = k * R and slot_words = R; timing->blocks_parsed counts the blocks of converted windows too.  frames of 2^55
 * and more: ACMHIP_ERR_ARG.
 * Where no row of a call converts - every file has C channels, or the others' windows deliver nothing - the launch is
 * acm_dense_rows as without the flag; else one launch of acm_dense_mixed (csrc/acm_dense_mix.hip) takes its place and writes the
 * plain rows as well.
 *
 * ACM_DENSE_RESAMPLE: files of several sample rates in one batch of rate Ro = dense->rate.  Without the flag nothing of the above
 * changes, and dense->rate and dense->reserved are not read: a caller built against the 16-byte acm_dense_opts stays correct.  With
 * it, rate == 0 or reserved != 0 is ACMHIP_ERR_ARG before anything is written.  The flag combines with ACM_DENSE_PLANAR,
 * ACM_DENSE_MIX and ACM_BATCH_PCM_F32.  For window k let Ri be the rate in its item's header, c_k the item's channel count after
 * force_chans, g = gcd(Ri, Ro), L = Ro / g, M = Ri / g.
 * As with ACM_DENSE_MIX a window's first_word and max_words count the item's OWN interleaved samples at its OWN rate; `whole`,
 * `words` (SOURCE samples) and `status` are what acm_batch_decode_windows reports for the same window, which delivers
 * f = words / c_k source frames.  The channel conversion comes first: x_ch[i], 0 <= i < f, is channel ch of source frame i AFTER the
 * conversion the row's mode defines above - a copy or a split for a file of C channels, (L + R) >> 1 or duplication with
 * ACM_DENSE_MIX; without ACM_DENSE_MIX a file of another channel count is turned away as ever.  (The down-mix floors, so the order
 * matters.)  x_ch[i] = 0 for i < 0 and i >= f: a row is the resampled CROP, the stream's own neighbours of the window are not used,
 * the windowed decode underneath is what it is without the flag and the kernel loads nothing but the row's own samples rounded out
 * to 16 bytes.
 * A row with Ri == Ro is exactly the row the call writes without the flag; it is not filtered.  A row of another rate has
 * n_out = ceil(f * L / M) = (f * L + M - 1) / M frames; frame j < n_out of channel ch, in the layout [T][C] or, with
 * ACM_DENSE_PLANAR, [C][T], is
 *   n = j * M;  base = n / L;  ph = n % L                                   (integer division)
 *   acc = sum over t in [0, K) of q[ph][t] * x_ch[base - Wd + 1 + t]        (32 bits; it cannot overflow, see the taps)
 *   y   = clamp((acc + 8192) >> 14, -32768, 32767)                          (arithmetic shift; it saturates, where the decoder wraps)
 * and the frames j >= n_out are zero.  float32 is y * 2^-15 exactly.  Every element of every row is written and nothing outside
 * [0, nwin * R), as without the flag.
 * The taps: Z = 8 zero crossings a side, a Hann-windowed sinc in Q14, computed on the host in double:
 *   s  = min(1, L / M)                                  the cutoff as a fraction of the source's Nyquist rate
 *   Wd = Z where L >= M, else (Z * M + L - 1) / L;      K = 2 * Wd
 *   for ph in [0, L), t in [0, K):   a = (t - Wd + 1) * L - ph;  u = a / L;  v = u * s / Z
 *       h[ph][t] = s * sinc(s * u) * (0.5 + 0.5 * cos(pi * v) where |v| < 1, else 0)        sinc(x) = sin(pi x) / (pi x), 1 at 0
 *   h[ph] /= sum over t of h[ph][t]
 *   q[ph][t] = nearbyint(h[ph][t] * 16384)                                 ties to even
 *   q[ph][first index of the largest q[ph]] += 16384 - sum over t of q[ph][t]
 * so every phase sums to 16384 exactly - a constant input comes out as it went in - and Ri == Ro has the single tap 16384, the
 * identity: why a row of the batch's rate may skip the filter.  Every phase has sum |q[ph][t]| < 65536, so |acc| < 2^31; the library
 * checks that of every table it designs.
 * A ratio is supported when Ri > 0, M <= 8 * L and L * K <= 16384, a table of 32 KB at most: 22050 -> 16000 (L 320, K 24),
 * 8000 -> 22050 (L 441, K 16), 48000 -> 11025 (L 147, K 70), 44100 <-> 48000.  A window whose item's ratio is not supported is
 * turned away softly, as one of another channel count without ACM_DENSE_MIX is: words = 0, status = ACMHIP_ERR_ARG, a row of
 * zeros, nothing of it parsed (timing->blocks_parsed shows it).  More than 16 distinct ratios among the resampled windows of one
 * call: ACMHIP_ERR_ARG for the whole call.
 * ACMHIP_ERR_ARG before anything is written where a window has first_word % c_k != 0, max_words % c_k != 0, or more frames than a
 * row takes: ceil((max_words / c_k) * L / M) > T for a resampled window, max_words / c_k > T for any other - so the longest source
 * window of a row is T * M / L frames.  Windows without a rate (not ACM, no such file, an unusable index), and those turned away
 * for their ratio or channel count, are checked as rows of the batch's own rate and deliver zeros.  frames of 2^40 and more:
 * ACMHIP_ERR_ARG.  dev_off = slot_off = k * R and slot_words = R as ever.
 * Where no row of a call resamples - every file is at Ro, the others' windows deliver nothing, or the flag is unset - the call
 * launches the kernel it launches without the flag, over the same row table, bit for bit.  Else one launch of acm_dense_resample
 * (csrc/acm_dense_resample.hip) takes its place and writes the plain and the converting rows as well; its second table (32 bytes a
 * row) and the ratios' taps travel behind the row table.
 *
 * ACM_DENSE_SPEED: a speed factor per window (speed perturbation), and any rate ratio.  It requires ACM_DENSE_RESAMPLE - alone it is
 * ACMHIP_ERR_ARG before anything is written - and combines with ACM_DENSE_PLANAR, ACM_DENSE_MIX and ACM_BATCH_PCM_F32.  Without the
 * flag nothing of the above changes: wins[k].reserved is not read and a ratio beyond the exact table is turned away.  With it, frames
 * of 2^28 and more are ACMHIP_ERR_ARG, and wins[k].reserved is the window's speed num << 16 | den, meaning num / den: 0 is 1 / 1,
 * exactly one half 0 is ACMHIP_ERR_ARG for the whole call.  num / den > 1 plays faster and gives fewer frames.  With Ri, Ro and c_k as
 * above, in 64 bits,
 *   g = gcd(Ri * num, Ro * den);  L = Ro * den / g;  M = Ri * num / g
 * take the place of the rates' L and M.  first_word and max_words still count the item's own samples, words and status are still
 * acm_batch_decode_windows', the channel conversion still comes first, samples outside the crop are zero, n_out = ceil(f * L / M),
 * and a window with n_out(max_words / c_k) > T - by its own L and M, computed without overflow - is ACMHIP_ERR_ARG for the whole
 * call.  With Wd and K of (L, M) as above, a row gets
 *   L == M                                   no filter: the row the call writes without the flags
 *   M <= 8 L and L * K <= 16384              the EXACT filter above, with the table of that (L, M), bit for bit: a table is a function
 *                                            of (L, M), so speed 9 / 10 at equal rates (L 10, M 9) is such a row
 *   M <= 8 L, L and M below 2^31, otherwise  the WIDE filter below
 *   anything else                            turned away softly: words = 0, ACMHIP_ERR_ARG, a row of zeros, nothing parsed
 * The wide filter has a table whose size does not depend on L: P + 1 prototype phases of the same windowed sinc, between two of which
 * the output is interpolated linearly, at a read position stepped in 32.32 fixed point.
 *   c  = 64 where L >= M, else floor(64 * L / M)       8 .. 63: the cutoff, quantised DOWN to 64ths of the source Nyquist;  s = c / 64
 *   Wd = Z where c == 64, else ceil(64 * Z / c);  K = 2 * Wd                                                    (16 .. 128)
 *   P  = the largest power of two with (P + 1) * K <= 16384;  b = log2 P       (K 16, 18: 512;  K 46: 256;  K 128: 64)
 *   for p in [0, P], t in [0, K):   u = (t - Wd + 1) - p / P;  v = u * s / Z
 *       h[p][t] = s * sinc(s * u) * (0.5 + 0.5 * cos(pi * v) where |v| < 1, else 0)
 *   h[p] /= sum over t of h[p][t];  q[p][t] = nearbyint(16384 * h[p][t]);  q[p][first index of the largest] += 16384 - sum over t of q[p][t]
 * The table depends on c alone - 57 tables at most, one for all upsampling ratios - and every phase has sum |q| < 65536 (33 588 at
 * most over the 57; the library checks every table it designs).  Output frame j < n_out of a channel is
 *   step = floor(M * 2^32 / L)                                      (below 2^36)
 *   X = j * step (64 bits unsigned; j < 2^28);  base = X >> 32;  frac = X & 0xFFFFFFFF
 *   p = frac >> (32 - b);  w = (frac >> (17 - b)) & 32767
 *   a0 = sum over t of q[p][t]     * x[base - Wd + 1 + t]
 *   a1 = sum over t of q[p + 1][t] * x[base - Wd + 1 + t]           (32-bit sums each)
 *   acc = a0 + (((a1 - a0) * w) >> 15)                              (in 64 bits; the shift arithmetic - the floor)
 *   y = clamp((acc + 8192) >> 14, -32768, 32767);  float32 = y * 2^-15
 * and the frames j >= n_out are zero.  step is rounded down, so the read position never runs ahead of the exact one j * M / L; it
 * falls behind by less than j * 2^-32 source frames: after 2^24 output frames by at most 2^-8 of one.
 * At most 16 distinct tables a call, exact (L, M) tables and wide c tables counted together; more is ACMHIP_ERR_ARG for the whole
 * call.  Windows without a rate, or turned away, are checked as rows of the batch's own rate at speed 1 and deliver zeros.
 * Where no row of a call is wide the call launches exactly what it launches without the flag, over the same tables.  Else one launch
 * of acm_dense_speed (csrc/acm_dense_speed.hip) takes its place and writes the exact-filtered, the converting and the plain rows as
 * well; its second table has 48 bytes a row.
 * ---------------------------------------------------------------------- */
#define ACM_DENSE_PLANAR   1u            /* row k is [channels][frames]; default [frames][channels] */
#define ACM_DENSE_MIX      4u            /* windows of files with the other channel count are converted, not turned away */
#define ACM_DENSE_RESAMPLE 16u           /* windows of files with another sample rate than dense->rate are resampled to it */
#define ACM_DENSE_SPEED    32u           /* wins[k].reserved is window k's speed; ratios beyond the exact table take the wide filter */
typedef struct acm_dense_opts {
	uint64_t frames;                 /* T >= 1 */
	uint32_t channels;               /* C: 1 or 2 (all an ACM header can say) */
	uint32_t flags;                  /* ACM_DENSE_* */
	uint32_t rate;                   /* Ro; read with ACM_DENSE_RESAMPLE only, and so is ... */
	uint32_t reserved;               /* ... this: 0 */
} acm_dense_opts;

/* frames of a row resampled from source_frames frames: n_out above, source_frames itself for equal rates; UINT64_MAX for a ratio that
 * is not supported (or 2^50 frames and more).  No device is needed */
uint64_t acm_dense_resampled_frames(uint64_t source_frames, uint32_t rate_in, uint32_t rate_out);
/* L, M, K, Wd (each may be NULL) and the Q14 table q[L][K] of a ratio into taps[cap] - what the kernel reads is this function's
 * output, uploaded.  taps == NULL: the sizes alone.  ACMHIP_ERR_ARG for a ratio that is not supported, or cap < L * K.  No device is
 * needed */
int  acm_dense_resample_taps(uint32_t rate_in, uint32_t rate_out, uint32_t *L, uint32_t *M, uint32_t *K, uint32_t *Wd, int16_t *taps,
			     size_t cap);

/* ACM_DENSE_SPEED's counterparts: a window of a file at rate_in played at num / den (both 1 .. 65535) into a batch at rate_out.  The
 * frames of its row - source_frames itself where L == M; UINT64_MAX where the window would be turned away (or 2^50 frames and more) */
uint64_t acm_dense_speed_frames(uint64_t source_frames, uint32_t rate_in, uint32_t rate_out, uint32_t num, uint32_t den);
typedef struct acm_dense_speed_info {
	uint32_t kind;                   /* 0: not filtered (L == M; L = M = 1 and the table is the identity's 16 taps), 1: exact, 2: wide */
	uint32_t L, M, K, Wd;
	uint32_t P, c;                   /* wide alone, else 0 */
	uint32_t phases;                 /* of the table: L, or P + 1 */
	uint64_t step;                   /* wide alone, else 0 */
} acm_dense_speed_info;
/* which filter the row gets (info may be NULL) and the table q[phases][K] the kernel reads into taps[cap]; taps == NULL: info alone.
 * ACMHIP_ERR_ARG where the window would be turned away, or cap < phases * K.  No device is needed */
int  acm_dense_speed_taps(uint32_t rate_in, uint32_t rate_out, uint32_t num, uint32_t den, acm_dense_speed_info *info, int16_t *taps,
			  size_t cap);

int  acm_batch_decode_windows_dense(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index,
				    acm_batch_window *wins, size_t nwin, const acm_batch_opts *opts,
				    const acm_dense_opts *dense, acm_window_timing *timing);

/* ------------------------------------------------------------------------
 * Dense crop batches with an overlay (csrc/acm_batch_windows.cpp over csrc/acm_overlay_layout.cpp, kernels:
 * csrc/acm_dense_overlay.hip): volume perturbation, and a second crop laid over the first at a chosen signal-to-noise ratio, in the
 * call that makes the batch.  A call of its own beside acm_batch_decode_windows_dense: that call's flags and what it does with them
 * are untouched.
 *
 * The nwin windows, opts and dense mean what they mean to acm_batch_decode_windows_dense - any of its flags, speeds in
 * wins[k].reserved included - and define nwin SOURCE ROWS S_k of R = frames * channels int16 elements: exactly the int16 rows that
 * call would write, a row of zeros for a window that delivers nothing or is turned away.  They go into memory of the handle's own,
 * not into opts->d_pcm.  opts->d_pcm receives nrows OUTPUT ROWS, row r at element r * R, int16 or (ACM_BATCH_PCM_F32) float32;
 * d_pcm_words >= nrows * R; every element of every output row is written and nothing outside [0, nrows * R).  The layout
 * (interleaved, or ACM_DENSE_PLANAR) is the sources': the operation is elementwise over the R elements of a row and knows no channels.
 *
 * Output row r, with A = S_a, B = S_b, G_MAX = 32768, on unbounded integers:
 *   SNR mode (b given, snr != 0)        Ea = sum over e < R of A[e]^2, Eb likewise - exact, both channels and the zeros behind a short
 *                                       crop included;  D = Eb * snr;  g = 0 if D == 0, else min(G_MAX, isqrt((Ea << 40) / D)):
 *                                       (g / 4096)^2 = Ea / (Eb * snr / 65536), the power ratio a : b that snr (Q16) asks for
 *   absolute mode (b given, snr == 0)   g = gain
 *   b == ACM_OVERLAY_NONE               g = 0
 *   m[e] = 4096 * A[e] + g * B[e]                                     (fits int32: |m| <= 2^27 + 2^30)
 *   y[e] = clamp((m[e] * vol + 2^23) >> 24, -32768, 32767)            (the product in 64 bits, the shift arithmetic; it saturates)
 * with vol == 0 meaning 4096; float32 is y * 2^-15 exactly.  vol == 4096 with b == ACM_OVERLAY_NONE is the identity.  a == b is
 * allowed, and so is a source used by many rows, a source used by none, and rows in any order.
 *
 * rows[r].gain (the g that was used), energy_a and energy_b (0 in absolute mode and without b) come back for every row.  wins[k].words
 * and .status are acm_batch_decode_windows_dense's; dev_off, slot_off and slot_words are 0: nothing of d_pcm belongs to a window.
 * nrows == 0 writes nothing to d_pcm and returns ACMHIP_OK.
 *
 * ACMHIP_ERR_ARG before anything is written: anything acm_batch_decode_windows_dense refuses for these windows and `dense`, with
 * d_pcm_words checked against nrows * R instead; rows == NULL with nrows > 0; a >= nwin; b >= nwin unless it is ACM_OVERLAY_NONE;
 * reserved != 0; vol > 65535; gain > 32768 in absolute mode; R >= 2^24 (so Ea << 40 stays below 2^94 and g^2 * D below 2^116).
 * dev == NULL: ACMHIP_ERR_NO_DEVICE.
 *
 * The dense run goes on unchanged up to its gather launch - whichever of its four kernels the call would have picked - which writes
 * int16 rows into the handle's source arena.  Behind it on the same stream: the energies zeroed, acm_dense_energy over the source
 * rows some row in SNR mode names (each summed once, integer atomics: reproducible), acm_dense_gains (g of every output row),
 * acm_dense_overlay over the output rows, and one read-back of 24 bytes a row.  timing->kernel_s spans synthesis through the combine.
 * ---------------------------------------------------------------------- */
#define ACM_OVERLAY_NONE 0xFFFFFFFFu
typedef struct acm_overlay_row {         /* one per OUTPUT row */
	uint32_t a;                      /* in:  source window, < nwin */
	uint32_t b;                      /* in:  source window laid over it, or ACM_OVERLAY_NONE */
	uint32_t vol;                    /* in:  Q12 gain on the sum, 1 .. 65535; 0 means 4096 */
	uint32_t snr;                    /* in:  power ratio a : b wanted, Q16, 1 .. 2^32-1; 0: `gain` is given (absolute mode) */
	uint32_t gain;                   /* in (absolute mode): Q12 gain of b, 0 .. 32768;  out: the g that was used, in either mode */
	uint32_t reserved;               /* 0 */
	uint64_t energy_a, energy_b;     /* out: the sums of squares g was made from; 0 in absolute mode and for b == ACM_OVERLAY_NONE */
} acm_overlay_row;

int  acm_batch_decode_windows_overlay(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index,
				      acm_batch_window *wins, size_t nwin, const acm_batch_opts *opts, const acm_dense_opts *dense,
				      acm_overlay_row *rows, size_t nrows, acm_window_timing *timing);
/* the g of SNR mode from two energies (the formula above on whatever it is given; snr == 0 gives 0).  No device is needed */
uint32_t acm_dense_overlay_gain(uint64_t energy_a, uint64_t energy_b, uint32_t snr);

/* ------------------------------------------------------------------------
 * Dense crop batches with an overlay and an impulse response (csrc/acm_batch_windows.cpp over csrc/acm_fir_layout.cpp, kernel:
 * csrc/acm_dense_fir.hip): reverberation - a source row convolved with a room impulse response before anything is laid over it.  A
 * call of its own beside acm_batch_decode_windows_overlay, which is untouched.
 *
 * Windows, opts, dense, rows and everything reported for them mean what they mean to acm_batch_decode_windows_overlay and define
 * source rows S_k of R = T * C int16 elements.  For a window k with p = fir->of_window[k] != ACM_FIR_NONE the source row the rest of
 * the call sees - the energies, the SNR gains, the combine - is F_k instead of S_k.  With h, ntaps, d = delay and s = shift of
 * fir->responses[p], on unbounded integers, channel by channel:
 *   x[i]   = channel ch of frame i of S_k for 0 <= i < T (planar: element ch * T + i; interleaved: i * C + ch), 0 elsewhere
 *   acc[j] = sum over t in [0, ntaps) of h[t] * x[j + d - t]                                0 <= j < T
 *   y[j]   = clamp((acc[j] + (s ? 1 << (s - 1) : 0)) >> s, -32768, 32767)                   (the shift arithmetic; it saturates)
 * F_k has the layout of S_k, and both channels of a stereo row get the same response.  The row is T frames whatever the crop
 * delivered: the tail of a short crop rings on into the zeros behind it, and what would fall behind frame T is cut.  d is the tap
 * that lands on the input's own position (the direct path).  A response is taken only if sum |h[t]| <= 65535: then |acc| < 2^31 and
 * a 32-bit accumulator is exact - acm_dense_fir_check is the one text of that check.  {h = [1], s = 0, d = 0} is the identity, and a
 * row of zeros stays a row of zeros.  The SNR energies are those of F_k: the noise is set against the reverberant speech.
 *
 * ACMHIP_ERR_ARG before anything is written: anything acm_batch_decode_windows_overlay refuses; responses == NULL or of_window ==
 * NULL with nresp > 0; nresp > 65536; reserved != 0; an entry of of_window >= nresp that is not ACM_FIR_NONE; a response that fails
 * acm_dense_fir_check (ntaps 0 or above 32768, delay >= ntaps, shift > 30, reserved != 0, sum |h| above 65535, taps == NULL); more
 * than 2^22 taps in the responses some window names, together.
 *
 * With fir == NULL, nresp == 0 or every entry ACM_FIR_NONE the call makes exactly the launches of acm_batch_decode_windows_overlay
 * over the same tables.  Else the source arena holds nwin + nfilt rows, F of the i-th filtered window in row nwin + i; one launch of
 * acm_dense_fir between the gather launch and the energy launch writes those rows, and the row table that is uploaded names them
 * where it named a filtered window - the caller's records keep their own a and b.  Responses no window names are not uploaded.
 * timing->kernel_s spans synthesis through the combine.
 * ---------------------------------------------------------------------- */
#define ACM_FIR_NONE 0xFFFFFFFFu
typedef struct acm_fir_response {
	const int16_t *taps;             /* h[0 .. ntaps), host memory */
	uint32_t ntaps;                  /* 1 .. 32768 */
	uint32_t delay;                  /* d < ntaps: the tap that lands on the input's own position */
	uint32_t shift;                  /* s, 0 .. 30 */
	uint32_t reserved;               /* 0 */
} acm_fir_response;
typedef struct acm_fir_opts {
	const acm_fir_response *responses;
	size_t nresp;                    /* <= 65536 */
	const uint32_t *of_window;       /* nwin entries: a response number, or ACM_FIR_NONE */
	uint64_t reserved;               /* 0 */
} acm_fir_opts;

int  acm_batch_decode_windows_overlay_fir(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index,
					  acm_batch_window *wins, size_t nwin, const acm_batch_opts *opts, const acm_dense_opts *dense,
					  const acm_fir_opts *fir, acm_overlay_row *rows, size_t nrows, acm_window_timing *timing);
/* ACMHIP_OK for a response the call takes, else ACMHIP_ERR_ARG.  No device is needed */
int  acm_dense_fir_check(const acm_fir_response *r);

/* ------------------------------------------------------------------------
 * Mel filterbank features from dense crop batches (csrc/acm_batch_windows.cpp over csrc/acm_feat_layout.cpp, kernels:
 * csrc/acm_dense_feat.hip): the speech front end - framing, window, DFT, power, mel filterbank - as part of the call that builds the
 * batch, so that the waveform never leaves the handle.  A call of its own beside acm_batch_decode_windows_overlay_fir, which is
 * untouched.
 *
 * Windows, opts, dense, fir, rows and everything reported for them (rows[], wins[], timing) mean what they mean to
 * acm_batch_decode_windows_overlay_fir and define nrows output rows Y_r of T int16 frames: exactly the int16 rows that call would
 * write.  They go into an arena of the handle's own ("D_FEAT" of acmhip_device_arena_info, filled with 0xA5 in fill mode like the
 * source arena), not to opts->d_pcm.  dense->channels must be 1 (ACM_DENSE_MIX makes mono rows of stereo files).  opts->d_pcm receives
 * float32 features whatever ACM_BATCH_PCM_F32 says, and opts->d_pcm_words counts float32 elements.
 *
 * With N = n_fft = 2^n, H = hop, B = n_mels, w = window, c = cs of `bank`, on unbounded integers, for a row x = Y_r with x[i] = 0
 * outside [0, T):
 *   frames    F = 1 + T / H with ACM_FEAT_CENTER (the division floors), else F = T >= N ? 1 + (T - N) / H : 0 (acm_feat_frames)
 *   start     frame f starts at s = f * H - (CENTER ? N / 2 : 0).  What lies outside the row is ZERO: torch.stft's
 *             pad_mode="constant", not its default "reflect"
 *   window    xw[t] = (x[s + t] * w[t] + 16384) >> 15, the shift arithmetic; w <= 32639 makes |xw| <= 32639, whose two signed
 *             bytes (v = 256 * hi + lo, lo the signed low byte) both fit int8
 *   DFT       for k in [0, N / 2]:  Re[k] =  sum over t of xw[t] * c[(k * t) mod N]
 *                                   Im[k] = -sum over t of xw[t] * c[(k * t + 3 N / 4) mod N]
 *   scaling   q = n - 1:  A = (Re + (1 << (q - 1))) >> q, Bv likewise from Im; |A|, |Bv| <= 2^30
 *   power     P[k] = A^2 + Bv^2 < 2^62
 *   mel       E[b] = sum over k in [mel_first[b], mel_first[b] + mel_count[b]) of mel_w[mel_off[b] + k - mel_first[b]] * P[k] < 2^89
 *   output    y = trunc24(E) * 2^-(75 - 2 n): trunc24 keeps the 24 leading bits of E and clears the rest, so y is an exact float32,
 *             needs no rounding mode and does not depend on the order of any sum
 * With the tables acm_feat_design makes, y is (32639 / 32768)^2 times - 0.034 dB below - the power mel spectrogram of x / 32768 under
 * a window of peak 1, up to quantisation.  This call writes the linear feature; acm_batch_decode_windows_logmel (below) writes its
 * logarithm, an integer one - a float log would not be bit-exact -, floored, clamped to the row's maximum and scaled, in the same run.
 *
 * Element (r, b, f) is at (r * B + b) * F + f, with ACM_FEAT_TIME_MAJOR at (r * F + f) * B + b.  Every element of [0, nrows * B * F)
 * is written and nothing outside; F == 0 or nrows == 0 writes nothing and is ACMHIP_OK.
 *
 * ACMHIP_ERR_ARG before anything is written: anything acm_batch_decode_windows_overlay_fir refuses; dense->channels != 1; a bank
 * acm_feat_bank_check refuses (bank or a table NULL, n_fft not 128, 256, 512, 1024 or 2048, hop 0 or above N, n_mels 0 or above
 * 128, unknown flags, reserved != 0, a window value outside [0, 32639], a cs value outside [-16384, 16384], a band reaching past bin
 * N / 2, a weight above 32768); opts->d_pcm_words < nrows * B * F.
 *
 * The run is acm_batch_decode_windows_overlay_fir's up to its combine launch, which writes int16 into the feature arena; then
 * acm_feat_twiddle builds the DFT's B operand from c - N x 2 * 16 * (N / 32 + 1) signed bytes twice, hi and lo, in the lane order of
 * v_mfma_i32_16x16x64_i8 - and acm_dense_feat makes the features: 16 frames of a row per workgroup, four matrix products
 * (hi.hi, hi.lo, lo.hi, lo.lo) per 16 x 16 tile, joined in 64 bits.  timing->kernel_s spans synthesis through the feature launch.
 * ---------------------------------------------------------------------- */
#define ACM_FEAT_CENTER     1u          /* frame f is centred on sample f * H; else it starts there and only whole frames count */
#define ACM_FEAT_TIME_MAJOR 2u          /* [row][frame][band] instead of [row][band][frame] */
#define ACM_FEAT_MAX_MELS   128u
#define ACM_FEAT_WINDOW_MAX 32639       /* 0x7F7F: then both signed bytes of a windowed sample fit int8 */
#define ACM_FEAT_CS_ONE     16384       /* c[m] stands for 16384 cos(2 pi m / N) */
#define ACM_FEAT_W_ONE      32768u      /* a mel weight of 1 (Q15) */
typedef struct acm_feat_bank {
	uint32_t n_fft;                  /* N: 128, 256, 512, 1024 or 2048; n = log2 N */
	uint32_t hop;                    /* H: 1 .. N */
	uint32_t n_mels;                 /* B: 1 .. 128 */
	uint32_t flags;                  /* ACM_FEAT_* */
	const int16_t *window;           /* w[N], 0 .. 32639 */
	const int16_t *cs;               /* c[N], -16384 .. 16384 */
	const uint16_t *mel_first, *mel_count;   /* per band: bins [first, first + count), inside [0, N / 2]; count 0 allowed */
	const uint32_t *mel_off;         /* per band: where its weights start in mel_w */
	const uint16_t *mel_w;           /* weights, 0 .. 32768 (Q15) */
	uint64_t reserved;               /* 0 */
} acm_feat_bank;

int  acm_batch_decode_windows_features(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index,
				       acm_batch_window *wins, size_t nwin, const acm_batch_opts *opts, const acm_dense_opts *dense,
				       const acm_fir_opts *fir, const acm_feat_bank *bank, acm_overlay_row *rows, size_t nrows, acm_window_timing *timing);
/* ACMHIP_OK for a bank the call takes, else ACMHIP_ERR_ARG: the one text of that check.  No device is needed */
int  acm_feat_bank_check(const acm_feat_bank *bank);
/* F of a row of T frames (only n_fft, hop and flags of the bank are read; 0 for a NULL bank or a hop of 0).  No device is needed */
uint64_t acm_feat_frames(uint64_t T, const acm_feat_bank *bank);
/* The tables of a mel spectrogram, written into the caller's storage: window[n_fft] - a periodic Hann of win_length <= n_fft samples
 * centred in n_fft, zeros around it, w = nearbyint(32639 * hann) -, cs[n_fft] - nearbyint(16384 * cos(2 pi m / N)) -, and n_mels
 * triangles between f_min and f_max (Hz, 0 <= f_min < f_max <= rate / 2) on the HTK mel scale 2595 log10(1 + f / 700), no area
 * normalisation, mel_w = nearbyint(32768 * weight), a band's range being its non-zero weights; mel_off[b] is the sum of the counts
 * in front of band b.  *n_weights receives the number of weights, whatever else is given.  Any of the table pointers may be NULL
 * (nothing is written there): a first call with all of them NULL reports the size of mel_w, as acm_dense_resample_taps does for its
 * taps.  ACMHIP_ERR_ARG for arguments out of range, or weights_cap < *n_weights with mel_w given.  No device is needed */
int  acm_feat_design(uint32_t rate, uint32_t n_fft, uint32_t win_length, uint32_t hop, uint32_t n_mels, double f_min, double f_max, uint32_t flags,
		     int16_t *window, int16_t *cs, uint16_t *mel_first, uint16_t *mel_count, uint32_t *mel_off, uint16_t *mel_w, size_t weights_cap,
		     size_t *n_weights);

/* ------------------------------------------------------------------------
 * Log-mel features (csrc/acm_batch_windows.cpp over csrc/acm_feat_layout.cpp, kernels: csrc/acm_dense_feat.hip):
 * acm_batch_decode_windows_features with the logarithm, a floor, the clamp to a row's maximum and an affine scale behind it - what
 * log10 / clamp / amax / maximum / (x + 4) / 4 of the usual recipes do in five launches more.  A call of its own beside
 * acm_batch_decode_windows_features, which is untouched; every argument but `log` means what it means there.
 *
 * The contract continues that call's, on unbounded integers: rows, frames, window, DFT, power, E[b], n = log2 N, the layouts and the
 * refusals are unchanged, and only its `output` line is replaced:
 *   mantissa  for E >= 1: p the position of E's leading bit, m in [2^23, 2^24) E's 24 leading bits (what trunc24 keeps; for p < 23
 *             they are shifted left)
 *   fraction  frac(m): x = m; sixteen times x = x * x, then bit = 1 and x >>= 24 if x >= 2^47, else bit = 0 and x >>= 23; frac is
 *             the sixteen bits, the first the highest.  x stays in [2^23, 2^24), frac is monotone in m, frac(2^23) = 0,
 *             frac(2^24 - 1) = 65535 and 0 <= 65536 * log2(m / 2^23) - frac(m) < 1.009 (all 2^23 mantissas: tests/test_dense_logmel.py)
 *   log       L = (p - (75 - 2 n)) * 65536 + frac(m): log2 of the linear feature y in Q16.  E = 0 gives L = floor_q16; then
 *             L = max(L, floor_q16)
 *   top       with ACM_FEAT_LOG_TOP: M_r = the maximum of L over all B * F elements of row r, and L = max(L, M_r - top_q16)
 *   scale     V = (((int64) L * mul_q24 + 2^23) >> 24) + offset_q16, the shift arithmetic
 *   output    the float32 V * 2^-16: |V| < 2^24 (acm_feat_log_check), so it is exact, needs no rounding mode and does not depend
 *             on the order of any sum or of the maximum
 * mul_q24 = 2^24 * c gives c * log2 y: c = ln 2 the natural logarithm, log10 2 the decimal one, 10 log10 2 decibels; the Whisper
 * recipe - log10, floor 1e-10, the maximum less 8, (x + 4) / 4 - is floor_q16 = nearbyint(65536 * log2(1e-10)), top_q16 =
 * nearbyint(65536 * 8 / log10 2), mul_q24 = nearbyint(2^24 * log10 2 / 4), offset_q16 = 65536.
 *
 * Every element of [0, nrows * B * F) is written and nothing outside; F == 0 or nrows == 0 writes nothing and is ACMHIP_OK.
 *
 * ACMHIP_ERR_ARG before anything is written: everything acm_batch_decode_windows_features refuses; log NULL; what acm_feat_log_check
 * refuses: unknown flags, reserved != 0, floor_q16 outside [-64 * 65536, 64 * 65536], mul_q24 outside [1, 2^28], top_q16 above
 * 128 * 65536 or not 0 without ACM_FEAT_LOG_TOP, or a setting whose |V| could reach 2^24 - with Lb = max(62 * 65536, |floor_q16|),
 * the largest |L| of any bank (p in [0, 88], n in [7, 11]), it requires ((Lb * mul_q24) >> 24) + |offset_q16| + 1 < 2^24.
 *
 * The run is acm_batch_decode_windows_features' with the logarithm in the feature kernel's last step, where E is in registers.
 * Without ACM_FEAT_LOG_TOP that is all, and the store is the final float.  With it the kernel stores L, a wavefront reduces its
 * maximum and adds it with one atomic maximum to a table of the handle's own (nrows int32 behind the DFT's operand in "D_FEAT", reset
 * by every call), and acm_feat_log_finish goes over the tensor once more, in place.  Nothing more is uploaded than for a features call.
 * ---------------------------------------------------------------------- */
#define ACM_FEAT_LOG_TOP       1u                       /* clamp to the row's maximum less top_q16 */
#define ACM_FEAT_LOG_FLOOR_MAX (64 * 65536)
#define ACM_FEAT_LOG_MUL_MAX   (1u << 28)
#define ACM_FEAT_LOG_TOP_MAX   (128u * 65536u)
typedef struct acm_feat_log {
	uint32_t flags;                  /* ACM_FEAT_LOG_TOP or 0 */
	int32_t  floor_q16;              /* the least L, log2 in Q16: -64 * 65536 .. 64 * 65536 */
	uint32_t mul_q24;                /* 1 .. 2^28 */
	int32_t  offset_q16;
	uint32_t top_q16;                /* 0 .. 128 * 65536; 0 without ACM_FEAT_LOG_TOP */
	uint32_t reserved;               /* 0 */
} acm_feat_log;

int  acm_batch_decode_windows_logmel(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index,
				     acm_batch_window *wins, size_t nwin, const acm_batch_opts *opts, const acm_dense_opts *dense,
				     const acm_fir_opts *fir, const acm_feat_bank *bank, const acm_feat_log *log, acm_overlay_row *rows, size_t nrows,
				     acm_window_timing *timing);
/* ACMHIP_OK for a bank and a scale the call takes, else ACMHIP_ERR_ARG: the one text of that check.  No device is needed */
int  acm_feat_log_check(const acm_feat_bank *bank, const acm_feat_log *log);

/* ------------------------------------------------------------------------
 * Batch index build (csrc/acm_batch_index.cpp): the block index of many files in one call - what acm_batch_decode_windows needs
 * before its first crop.  acm_index_file parses a whole file to get it, decoding every filler index and dropping it; the device
 * only WALKS the stream (acm_index_scan_wave, csrc/acm_parse.hip: one stream per wavefront, the walk of acm_batch_decode's device
 * parser without its column offsets), validates the ternary columns it skips by length, and writes one acm_block_mark per block:
 * 16 bytes of device memory per block beside the file image, nothing per column or per sample.
 *
 * For every item, marks[0 .. blocks], blocks, end_status and status are byte for byte what
 * acm_index_file(data, len, force_chans, marks, max_blocks, &info) writes and returns (info.blocks, info.end_status, the return
 * code), whoever did the work.  The device takes the clean streams; a stream it flags (data running out, an invalid filler code,
 * a ternary symbol out of range), whose walk ends short of the blocks the header promises, whose last mark lies behind the end
 * of the file, or that the layout kept off the device (not ACM, no room for marks, a file of 256 MiB or more, a header that
 * promises more blocks than the bytes can hold, unless max_blocks asks for fewer than they could hold) goes to the host pool, which runs acm_index_file on it while later groups are
 * still on the device.  A dirty stream never fails the call.  H1 does not matter to an index: such streams stay on the device.
 *
 * The batch travels in groups (csrc/acm_index_layout.cpp: file bytes + marks of a group <= opts->max_group_bytes, at most 32768
 * streams); the upload of group k + 1 overlaps the walk of group k, so the device holds two groups at most.
 *
 * opts->parse:
 *   ACM_BATCH_PARSE_HOST    the pool only; dev may be NULL (a box without a GPU).
 *   ACM_BATCH_PARSE_DEVICE  the device walk for every stream the layout lets it have; dev == NULL: ACMHIP_ERR_NO_DEVICE.
 *   ACM_BATCH_PARSE_AUTO    DEVICE when the batch is worth at least 12 x threads streams of its longest stream's size (192 at 16 threads),
 *                           HOST below that and when dev is NULL.  Measured on an MI355X with 16 host threads
 *                           (profiles/index_build_notes.txt): a launch of the walk lasts as long as its longest stream however many
 *                           streams it has - 35 ms for 2 Msamples -, so the pool wins small batches (256 files of the 4000-file
 *                           corpus, 47 streams' worth: 15 against 48 ms), the two meet at 1024 of its files (196 streams' worth,
 *                           56 against 60 ms) and the device is ahead beyond: the whole corpus 116 against 338 ms for the host parser
 *                           (batch.build_index), 1024 level-9 streams of 250 blocks 70 against 232 ms.
 * opts == NULL: AUTO, the library's group size, one thread per CPU.
 * ---------------------------------------------------------------------- */
typedef struct acm_batch_index_out {     /* one per item */
	acm_block_mark *marks;           /* in:  room for max_blocks + 1 marks */
	size_t   max_blocks;             /* in */
	uint32_t blocks;                 /* out: acm_stage_info.blocks of acm_index_file */
	int32_t  end_status;             /* out: acm_stage_info.end_status of acm_index_file */
	int32_t  status;                 /* out: what acm_index_file returns for this item: ACM_OK, ACM_ERR_NOT_ACM, ACMHIP_ERR_ARG */
	uint32_t reserved;
} acm_batch_index_out;

typedef struct acm_index_opts {
	int      force_chans;
	int      threads;                /* host pool, 0 = one per CPU */
	unsigned parse;                  /* ACM_BATCH_PARSE_* */
	unsigned reserved;
	uint64_t max_group_bytes;        /* file bytes + marks of one group on the device; 0 = the library decides (1 GiB: every group costs
	                                    the walk of its longest stream again, groups only bound the memory) */
} acm_index_opts;

typedef struct acm_index_timing {
	double   stage_s;                /* host time spent filling the pinned file arena and the job tables */
	double   h2d_s, kernel_s, d2h_s; /* device-side durations summed over the groups (they overlap each other and the host pool) */
	double   total_s;                /* wall clock of the whole call */
	uint64_t blocks;                 /* blocks indexed, by anyone */
	uint64_t device_indexed;         /* items whose marks are the device walk's ... */
	uint64_t host_indexed;           /* ... and items acm_index_file ran on (the two add up to n) */
	uint64_t h2d_bytes;              /* file images and job tables sent to the device */
	uint64_t device_bytes;           /* device memory the call worked in: two groups of file slots, marks, jobs and results */
	uint32_t groups;
	uint32_t reserved;
} acm_index_timing;

/* blocks to make room for: per_item[i] (may be NULL) = the max_blocks that lets item i's whole index fit (the blocks its header
 * promises, but no more than its bytes can hold; 0 for a file that is not ACM) - marks takes one entry more.  Returns their sum. */
uint64_t acm_batch_index_blocks(const acm_batch_item *items, size_t n, int force_chans, uint64_t *per_item);
/* items: data / len are read, nothing is written.  out[i] belongs to items[i]. */
int  acm_batch_index_files(acmhip_device *dev, const acm_batch_item *items, size_t n, acm_batch_index_out *out,
			   const acm_index_opts *opts, acm_index_timing *timing);

/* ------------------------------------------------------------------------
 * The block index as a by-product of a whole decode (csrc/acm_batch.cpp): whoever bit-parses a stream for acm_batch_decode stands
 * on the first bit of every block and reads its (val, pwr), so a data set that is decoded whole once has paid for its index.
 *
 * acm_batch_decode_indexed with index == NULL is acm_batch_decode.  With n entries of index, items, PCM, offsets, statuses and
 * *timing are exactly what acm_batch_decode gives for the same arguments, and for every item index[i].marks[0 .. blocks], blocks,
 * end_status and status are byte for byte what acm_index_file(data, len, force_chans, marks, B_i, &info) writes and returns, B_i
 * being the item's per_item value of acm_batch_index_blocks() - the blocks the decode stages.  marks behind blocks + 1 entries are
 * not written; a file that is not ACM leaves its marks untouched.  index[i].marks == NULL or index[i].max_blocks < B_i for an item
 * that is ACM: ACMHIP_ERR_ARG before anything is written.
 *
 * Nobody parses a stream for the index who would not have parsed it anyway (timing->device_parsed / host_parsed are those of
 * acm_batch_decode): the device walk (acm_parse_scan_wave whole or in block ranges, acm_parse_scan beyond 32768 streams) stores a
 * 16-byte mark beside every block header it stores - 16 bytes of device memory per block, read back once behind the last walk -,
 * the host pool's stagers and the redo of a stream the device flagged write the caller's marks where they begin a block, and a
 * prestaged batch hands over the marks acm_batch_prestage kept.
 * ---------------------------------------------------------------------- */
int  acm_batch_decode_indexed(acmhip_device *dev, acm_batch_item *items, size_t n, const acm_batch_opts *opts,
			      acm_batch_index_out *index /* n entries, or NULL */, acm_batch_timing *timing);
/* The index of item i of a prestaged batch, no device: *marks (blocks + 1 entries inside p, valid until acm_batch_prestage_free; NULL
 * for a file that is not ACM), *blocks and *end_status as acm_index_file gives them for the item's acm_batch_index_blocks() blocks.
 * Returns the item's acm_index_file code, or ACMHIP_ERR_ARG for an i that p does not have. */
int  acm_batch_prestaged_index(const acm_batch_prestaged *p, size_t i, const acm_block_mark **marks, uint32_t *blocks, int32_t *end_status);

#ifdef __cplusplus
}
#endif
#endif
