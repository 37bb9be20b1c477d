/*
 * acm_batch_layout.h - where everything of a batch goes and which way every stream travels, decided on the host from the
 * headers, the file lengths and the options alone.  Internal.  Neither this header nor acm_batch_layout.cpp knows a device
 * (tests/test_batch_layout.py); acm_batch.cpp drives the device over a BatchLayout it never modifies.
 */
#ifndef ACM_BATCH_LAYOUT_H
#define ACM_BATCH_LAYOUT_H

#include <algorithm>
#include <vector>

#include "acm_device.h"

namespace acmbatch {

inline uint64_t round_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

/* a file's slot of the file arenas: padded to 16 bytes, 16 zero bytes behind it (the device readers load whole dwords) */
inline uint64_t file_slot_bytes(uint64_t len) { return round_up(len, 16) + 16; }

/* Blocks a file can possibly hold: the header promises total_values, but arenas are sized by this - a block costs at
 * least its 20-bit header and a 5-bit filler code per column (decode.c:491-502, 586-589), and the reader appends one
 * virtual zero byte (decode.c:57-61).  A 19-byte file that claims 2^32-1 samples gets one block, not 8 GB. */
inline uint64_t blocks_possible(const acm_stage_info &info, size_t len)
{
	const uint64_t bl = (uint64_t)info.rows * info.cols;
	const uint64_t promised = ((uint64_t)info.total_values + bl - 1) / bl;
	const uint64_t bits = (len > info.header_bytes ? (uint64_t)(len - info.header_bytes) * 8 : 0) + 8;
	return std::min<uint64_t>(promised, bits / (20 + 5 * (uint64_t)info.cols) + 1);
}

/* How many words a caller looping over acm_read_loop() (acmtool.c:274-291)
 * gets out of `blocks` decodable blocks: blocks are drained whole except where
 * the per-call rounding to a multiple of `channels` (decode.c:856-857) or the
 * total_values cut (decode.c:853-854) stops the stream for good. */
inline uint64_t deliverable_words(uint64_t total_values, uint64_t block_len, unsigned channels, uint64_t blocks)
{
	uint64_t pos = 0;
	for (uint64_t b = 0; b < blocks && pos < total_values; b++) {
		uint64_t take = std::min(block_len, total_values - pos);
		if (channels > 1)
			take -= take % channels;
		pos += take;
		if (take != block_len)
			break;
	}
	return pos;
}

/* what the layout is computed from, per item: the probed header, whether the probe took the file, its length, whether the caller
 * gave a PCM buffer */
struct LayoutItem {
	acm_stage_info info{};
	uint64_t len = 0;
	bool ok = false, has_pcm = false;
};

struct SlotLayout {
	uint64_t need_blocks = 0;
	uint64_t idx_off = 0, hdr_off = 0, pcm_off = 0;
	uint64_t idx_len = 0;           /* arena words reserved (multiple of 64) */
	uint32_t chunk = 0;
	/* ACM_BATCH_STAGE_PACKED: the stream's chunk-table entries (reserved from the headers) */
	uint64_t pk_chunk_off = 0, pk_chunk_cap = 0;
	/* the device parser writes the byte-plane form: the whole tiles it stages that way (else 0: the host pool decides as it parses) */
	uint32_t pk_ntiles = 0;
	/* ACM_BATCH_STAGE_BYTEPLANE: where the stream's byte-plane block sits in the blob arena (bytes), how many rows it may hold, and
	 * its first entry in the pair table */
	uint64_t mf_off = 0, mf_rows_cap = 0, mf_pair_off = 0;
	uint32_t range_unit = 1;        /* device parsing in block ranges: the stream's ranges are cut at multiples of this many blocks (acmk_range_bound) */
	uint64_t file_off = 0;          /* device parsing: its slot of the file arenas */
	bool on_dev = false;            /* handed to the device parser */
};

/* a run of whole streams that travels through the device as one unit */
struct ChunkLayout {
	size_t first = 0, last = 0;             /* stream index range [first, last) */
	uint64_t idx_begin = 0, idx_end = 0;    /* arena ranges (int16 units; the PCM arena has the same layout) */
	uint64_t hdr_begin = 0, hdr_end = 0;
	uint64_t pk_chunk_begin = 0, pk_chunk_end = 0;  /* ACM_BATCH_STAGE_PACKED: its range of the chunk table (entries) */
	uint64_t mf_begin = 0, mf_end = 0;              /* ACM_BATCH_STAGE_BYTEPLANE: its range of the blob arena (bytes) */
	uint64_t mf_pair_begin = 0, mf_pair_end = 0;    /* ... and of the pair table (entries) */
};

/* device parsing: the files of one chunk as an upload piece */
struct GroupLayout {
	size_t k_first = 0, k_last = 0;         /* range of the device-parsed streams (indices into dev_ids) */
	uint64_t file_begin = 0, file_end = 0;  /* bytes of the file arenas */
	uint64_t max_columns = 0;
};

struct BatchLayout {
	std::vector<SlotLayout> slots;
	std::vector<ChunkLayout> chunks;
	std::vector<GroupLayout> groups;        /* one per chunk with device parsing, else none */
	std::vector<size_t> dev_ids;            /* streams handed to the device parser */
	std::vector<size_t> host_ids;           /* streams the host pool parses; ascending, i.e. arena order */
	std::vector<size_t> out_ids;            /* streams the pool copies out of the library's PCM arena */
	std::vector<AcmParseJob> jobs;          /* [k]: the device parser's job for stream dev_ids[k] */
	/* block ranges: [r * n + i] = where range r of stream i sits in the PCM arenas (words); rbase[r] = where range r begins */
	size_t R = 1;
	std::vector<uint64_t> piece_off, piece_len, rbase;
	/* ... and [s * nd + k] = stripe s of stream dev_ids[k] in the striped file arenas; stripe_base[s] = where stripe s begins */
	std::vector<uint64_t> stripe_at, stripe_base;
	uint64_t idx_total = 0, hdr_total = 0, pcm_total = 0, pcm_arena_words = 0;
	uint64_t pk_chunks_total = 0, mf_total = 0, mf_pairs_total = 0, files_total = 0, cols_total = 0;
	/* the H_JOBS / D_JOBS arena: the jobs, the results and their flags (res_bytes, from jobs_bytes on), the stripe table */
	size_t jobs_bytes = 0, res_bytes = 0, stripe_tab_off = 0, stripe_tab_bytes = 0;
	/* the way the batch travels, resolved once */
	bool stage_packed = false;      /* host parsing: the pool packs whole tiles (acmhip_pack_tiles) */
	bool stage_mform = false;       /* host parsing: the pool writes the byte-plane form */
	bool dev_parse = false;         /* the device parser takes the streams it can */
	bool dev_mform = false;         /* ... and writes the byte-plane form itself */
	bool direct_out = false;        /* the copy engine writes into the callers' pinned buffers */
	bool keep_on_device = false;    /* PCM stays in opts.d_pcm */
};

/* the int16 arenas of a batch (staged indices and PCM alike; block headers beside them): decodable stream after stream, each padded
 * to 64 words.  Shared by acm_batch_pcm_words, acm_batch_prestage and the layout */
struct Int16Arenas {
	uint64_t idx_total = 0, hdr_total = 0;
	/* the next stream's slices; returns the words reserved for it */
	uint64_t place(const acm_stage_info &info, uint64_t len, uint64_t *need_blocks, uint64_t *idx_off, uint64_t *hdr_off)
	{
		*need_blocks = blocks_possible(info, len);
		const uint64_t idx_len = round_up(*need_blocks * (uint64_t)info.rows * info.cols, 64);
		*idx_off = idx_total;
		*hdr_off = hdr_total;
		idx_total += idx_len;
		hdr_total += *need_blocks;
		return idx_len;
	}
};

/* does the device parser write this level's streams in the byte-plane form (the chunk kernel's levels)? */
bool lean_form_level(uint32_t level);

/* ACMHIP_OK, or ACMHIP_ERR_ARG (opts.d_pcm too small); `out` is a fresh BatchLayout.  prestaged: opts.prestaged is set (the items are
 * parsed already: ACM_BATCH_PARSE_HOST semantics, no second form unless asked for) */
int acm_batch_layout(const LayoutItem *items, size_t n, const acm_batch_opts &opts, int threads_wanted, bool prestaged, BatchLayout *out);

} // namespace acmbatch

extern "C" {
/* The layout shown to a visitor, table by table (tests): `visit` is called once per non-empty table with its name - slots (16 words
 * per item: the SlotLayout fields in order, then ok), chunks (12 words), groups (5 words), dev_ids, host_ids, out_ids, jobs (AcmParseJob),
 * piece_off, piece_len, rbase, stripe_at, stripe_base - then once with "totals": idx_total, hdr_total, pcm_total, pcm_arena_words,
 * pk_chunks_total, mf_total, mf_pairs_total, files_total, cols_total, jobs_bytes, res_bytes, stripe_tab_off, stripe_tab_bytes, R,
 * stage_packed, stage_mform, dev_parse, dev_mform, direct_out, keep_on_device and the return code, as uint64 words.  An item is
 * info[i], len[i], ok[i], has_pcm[i].  Returns acm_batch_layout's code; nothing is visited unless that is ACMHIP_OK */
typedef void (*acmk_layout_visit)(void *ctx, const char *table, const void *data, size_t elem_bytes, size_t count);
int acmk_batch_layout_visit(const acm_stage_info *info, const uint64_t *len, const uint8_t *ok, const uint8_t *has_pcm, size_t n,
			    const acm_batch_opts *opts, int threads_wanted, int prestaged, acmk_layout_visit visit, void *ctx);
}

#endif
