/*
 * acm_stage.cpp - the host stagers of a file image held in memory (include/acm_hip.h): the block index, whole files as int16 rows or
 * in the byte-plane form, and a run of blocks entered through the index.  One reader and one block loop; the stagers differ in where a
 * block's indices go and in what they do with a whole block.  No device code here.
 *
 * An ACM stream has no index of its own: where block b starts is known only once every block in front of it has been parsed
 * (decode.c:478-502).  But a block depends on the blocks in front of it in two ways only - where it starts, and what they left
 * in the never-cleared amplitude table (hazard H1, decode.c:809-810), which is a function of their (pwr, val) headers alone
 * (acmfill::TableHistory).  16 bytes per block - start bit, val, pwr - therefore let a reader enter the stream at any block and
 * produce exactly what a reader that came all the way from the header produces.
 */
#include "acm_stage.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "acm_device.h"
#include "acm_fill.h"
#include "acm_mform.h"

namespace {

using acmstage::MarkSink;

struct Source {
	const uint8_t *p;
	size_t len, pos;
};

int source_read(void *ptr, int size, int n, void *arg)
{
	Source *m = (Source *)arg;
	size_t want = (size_t)size * (size_t)n;
	if (want > m->len - m->pos)
		want = m->len - m->pos;
	memcpy(ptr, m->p + m->pos, want);
	m->pos += want;
	return size ? (int)(want / (size_t)size) : 0;
}

struct Reader {
	ACMStream a;
	Source src;
	acmfill::TableHistory tab;
	Reader() { memset(&a, 0, sizeof(a)); }
	~Reader() { free(a.buf); }
	int open(const uint8_t *data, size_t len, int force_chans)
	{
		src = Source{ data, len, 0 };
		tab.reset();
		a.io.read_func = source_read;
		a.io_arg = &src;
		a.data_len = (unsigned)len;
		a.buf_max = acmfill::kChunkBytes;
		a.buf = (unsigned char *)malloc(a.buf_max);
		if (!a.buf)
			return ACM_ERR_OTHER;
		return acmfill::open_common(&a, force_chans);
	}
	uint64_t bit() const { return MarkSink::bit(a); }
	uint64_t blocks_promised() const { return ((uint64_t)a.total_values + a.block_len - 1) / a.block_len; }
	/* Put the reader where one that came from the start of the file is when it stands at `at` (a bit inside the file): that reader
	 * takes the file in chunks of kChunkBytes from offset 0 and its accumulator in dwords from offset 0 (decode.c:69-135), and what it
	 * does in the last bytes of a file - the partial dword, the one zero byte behind the end - depends on both. */
	int enter(uint64_t at)
	{
		const size_t byte = (size_t)(at >> 3) & ~(size_t)3;
		const size_t chunk = byte & ~(size_t)(acmfill::kChunkBytes - 1);
		const size_t n = std::min<size_t>(acmfill::kChunkBytes, src.len - chunk);
		memcpy(a.buf, src.p + chunk, n);
		src.pos = chunk + n;
		a.buf_size = (unsigned)n;
		a.buf_pos = (unsigned)(byte - chunk);
		a.buf_start_ofs = (unsigned)chunk;
		a.file_eof = 0;
		a.bit_avail = 0;
		a.bit_data = 0;
		return acmfill::skip_bits(&a, (unsigned)(at - 8ull * byte));
	}
};

struct LoopEnd {
	uint64_t b;             /* the block the loop stopped in front of or in: blocks [first, b) are whole */
	int status;             /* 0: all of them, or the data ended at a block boundary; else what stopped it */
};

/* The block loop of every stager: blocks [first, want) from where the reader stands.  dest(b) says where block b's indices go (and
 * sets the patch sink up for it), whole(b, header) takes a block that parsed whole and returns 0, or a status that ends the loop with
 * that block not counted.  hdr: headers go to hdr[b]; null: to a scratch header only whole() sees */
template <class Dest, class Whole>
LoopEnd parse_blocks(Reader &c, uint64_t first, uint64_t want, acmhip_blkhdr *hdr, acmfill::PatchSink &sink, const MarkSink &mk, Dest dest,
		     Whole whole)
{
	acmhip_blkhdr scratch;
	uint64_t b = first;
	int status = 0;
	for (; b < want; b++) {
		acmhip_blkhdr *const h = hdr ? hdr + b : &scratch;
		mk.begin(b, c.a);
		const int rc = acmfill::parse_block(&c.a, &c.tab, dest(b), h, &sink);
		if (rc != 1) {
			status = (rc == acmfill::kCleanEof) ? 0 : rc;
			break;
		}
		mk.whole(b, *h);
		status = whole(b, *h);
		if (status != 0)
			break;
	}
	mk.end(b, b == want, c.a);
	return LoopEnd{ b, status };
}

void finish(acm_stage_info *info, uint64_t blocks, int status, uint64_t npatches)
{
	info->blocks = (uint32_t)blocks;
	info->end_status = status;
	info->npatches = npatches;
}

/* acm_stage_file into out->info and out->patches */
int stage_plain(const uint8_t *data, size_t len, int force_chans, int16_t *idx, acmhip_blkhdr *hdr, size_t max_blocks, acm_block_mark *marks,
		acmstage::Staged *out)
{
	out->info = acm_stage_info{};
	out->patches.clear();
	Reader c;
	const int rc = c.open(data, len, force_chans);
	if (rc < 0)
		return rc;
	acmfill::fill_stage_info(&c.a, &out->info);
	const size_t bl = c.a.block_len;
	acmfill::PatchSink sink{ &out->patches, 0, 0, 0 };
	const LoopEnd e = parse_blocks(
		c, 0, std::min<uint64_t>(c.blocks_promised(), max_blocks), hdr, sink, MarkSink{ marks },
		[&](uint64_t b) {
			sink.base_sample = b * bl;
			return idx + b * bl;
		},
		[](uint64_t, const acmhip_blkhdr &) { return 0; });
	finish(&out->info, e.b, e.status, out->patches.size());
	return ACM_OK;
}

/*
 * The same with the byte-plane form written while the parsed block is still in the cache: a block is parsed into a buffer of its own
 * (16 KB at level 9: the first-level cache, where the column scatter of the parser costs nothing), its row pairs go to the byte-plane
 * writer from there, and only the rows the int16 kernels still read - from two rows in front of the ragged tail on - are copied to
 * idx.  Against acm_stage_file + acmhip_mform_rows this drops the 2 B per sample written to and read back from the int16 arena.
 * 1: rows [0, out->mf_rows) are in the form (whole tiles of the lean kernel) and out is complete.  0: the stream has none (a level
 * without the form, H1 patches, an index beyond the form's range, a file that ends early) and has to be staged the plain way, from its
 * header again; whatever this attempt has written by then, the plain way writes again.  Negative: the file did not open
 */
int stage_fused(const uint8_t *data, size_t len, int force_chans, int16_t *idx, acmhip_blkhdr *hdr, size_t max_blocks, acm_block_mark *marks,
		const acmstage::MformArena &mf, acmstage::Staged *out)
{
	Reader c;
	const int rc = c.open(data, len, force_chans);
	if (rc < 0)
		return rc;
	acm_stage_info *const info = &out->info;
	acmfill::fill_stage_info(&c.a, info);
	const uint32_t level = info->level, rows = info->rows;
	const int T2 = acmk_tile2_rows(level), TM = acmhip_mform_tile_rows(level);
	/* (levels 13 / 14: whether a plan takes such a stream's form is known only from the whole plan - acmhip_plan_form_rows - so its
	 * int16 rows may all be needed: the plain way) */
	if (!mf.out || !mf.pairs || T2 <= 0 || TM <= 0 || T2 % TM || level > ACM_K1_MAX_LEVEL)
		return 0;
	const size_t bl = c.a.block_len, cols = (size_t)1 << level;
	const uint64_t want = std::min<uint64_t>(c.blocks_promised(), max_blocks);
	/* what a complete file delivers (decode.c:853-857: whole blocks, the last one cut at total_values, rounded to whole frames) */
	auto deliverable = [&](uint64_t blocks) {
		uint64_t pos = 0;
		for (uint64_t b = 0; b < blocks && pos < c.a.total_values; b++) {
			uint64_t take = std::min<uint64_t>(bl, c.a.total_values - pos);
			if (info->channels > 1)
				take -= take % info->channels;
			pos += take;
			if (take != bl)
				break;
		}
		return pos;
	};
	const uint64_t rows2 = std::min<uint64_t>(want * rows, deliverable(want) >> level) / (uint64_t)T2 * (uint64_t)T2;
	if (rows2 == 0)
		return 0;
	const uint64_t tail_from = rows2 >= 2 ? rows2 - 2 : 0;
	std::vector<int16_t> block(bl), straddle((rows & 1) ? 2 * cols : 0);
	AcmMformWriter w;
	if (acm_mform_begin(&w, level, mf.out, mf.base, mf.pairs) != ACMHIP_OK)
		return 0;
	acmfill::PatchSink sink{ nullptr, 0, 0, 0 };
	const LoopEnd e = parse_blocks(
		c, 0, want, hdr, sink, MarkSink{ marks }, [&](uint64_t) { return block.data(); },
		[&](uint64_t b, const acmhip_blkhdr &) {
			if (sink.count)
				return ACM_ERR_OTHER;           /* H1: the stream keeps the int16 form */
			const uint64_t r0 = b * rows;
			/* row pairs count from the stream's row 0: with an odd acm_rows every other block starts on the second row of a pair, whose
			 * first row is the last one of the block before (kept in `straddle`) */
			for (uint32_t r = 0; r < rows && r0 + r < rows2;) {
				const int16_t *two = block.data() + (size_t)r * cols;
				if ((r0 + r) & 1) {
					memcpy(straddle.data() + cols, two, cols * sizeof(int16_t));
					two = straddle.data();
					r += 1;
				} else if (r + 1 < rows) {
					r += 2;
				} else {
					if (straddle.empty())
						straddle.resize(2 * cols);
					memcpy(straddle.data(), two, cols * sizeof(int16_t));
					break;
				}
				if (acm_mform_put_pair(&w, two) != ACMHIP_OK)
					return ACM_ERR_OTHER;   /* an index beyond the form's range */
			}
			if (r0 + rows > tail_from) {
				const uint32_t from = r0 >= tail_from ? 0u : (uint32_t)(tail_from - r0);
				memcpy(idx + (r0 + from) * cols, block.data() + (size_t)from * cols, (size_t)(rows - from) * cols * sizeof(int16_t));
			}
			return 0;
		});
	if (e.b != want || deliverable(e.b) != deliverable(want))
		return 0;                           /* stopped, or the file ends early: fewer whole tiles than its header promised */
	finish(info, e.b, e.status, 0);
	out->mf_rows = rows2;
	out->mf_bytes = acm_mform_end(&w);
	return 1;
}

} // namespace

int acmstage::stage_file(const uint8_t *data, size_t len, int force_chans, int16_t *idx, acmhip_blkhdr *hdr, size_t max_blocks,
			 acm_block_mark *marks, const MformArena *mf, Staged *out)
{
	if (!data || !out || (max_blocks && (!idx || !hdr)))
		return ACMHIP_ERR_ARG;
	*out = Staged{};
	if (mf) {
		const int fused = stage_fused(data, len, force_chans, idx, hdr, max_blocks, marks, *mf, out);
		if (fused != 0)
			return fused < 0 ? fused : ACM_OK;
	}
	return stage_plain(data, len, force_chans, idx, hdr, max_blocks, marks, out);
}

extern "C" int acm_stage_probe(const uint8_t *data, size_t len, int force_chans, acm_stage_info *info)
{
	if (!data || !info)
		return ACMHIP_ERR_ARG;
	memset(info, 0, sizeof(*info));
	Reader c;
	const int rc = c.open(data, len, force_chans);
	if (rc < 0)
		return rc;
	acmfill::fill_stage_info(&c.a, info);
	return ACM_OK;
}

extern "C" int acm_stage_file(const uint8_t *data, size_t len, int force_chans, int16_t *idx, acmhip_blkhdr *hdr, size_t max_blocks,
			      acmhip_patch *patches, size_t max_patches, acm_stage_info *info)
{
	if (!data || !info || (max_blocks && (!idx || !hdr)) || (max_patches && !patches))
		return ACMHIP_ERR_ARG;
	acmstage::Staged st;
	const int rc = acmstage::stage_file(data, len, force_chans, idx, hdr, max_blocks, nullptr, nullptr, &st);
	*info = st.info;
	const size_t ncopy = std::min(st.patches.size(), max_patches);
	if (rc == ACM_OK && ncopy)
		memcpy(patches, st.patches.data(), ncopy * sizeof(acmhip_patch));
	return rc;
}

extern "C" int acm_stage_file_mform(const uint8_t *data, size_t len, int force_chans, int16_t *idx, acmhip_blkhdr *hdr, size_t max_blocks,
				    acm_stage_info *info, uint8_t *mf_out, uint64_t mf_base, acmhip_mform_pair *pairs, uint64_t *mf_rows,
				    uint64_t *mf_bytes)
{
	if (!data || !info || !mf_rows || !mf_bytes || (max_blocks && (!idx || !hdr)))
		return ACMHIP_ERR_ARG;
	acmstage::Staged st;
	const acmstage::MformArena mf{ mf_out, mf_base, pairs };
	const int rc = acmstage::stage_file(data, len, force_chans, idx, hdr, max_blocks, nullptr, &mf, &st);
	*info = st.info;
	*mf_rows = st.mf_rows;
	*mf_bytes = st.mf_bytes;
	return rc;
}

extern "C" int acm_index_file(const uint8_t *data, size_t len, int force_chans, acm_block_mark *marks, size_t max_blocks,
			      acm_stage_info *info)
{
	if (!data || !info || !marks)
		return ACMHIP_ERR_ARG;
	memset(info, 0, sizeof(*info));
	Reader c;
	const int rc = c.open(data, len, force_chans);
	if (rc < 0)
		return rc;
	acmfill::fill_stage_info(&c.a, info);
	std::vector<int16_t> block(c.a.block_len);              /* the indices are parsed (H1 is counted) and dropped */
	acmfill::PatchSink sink{ nullptr, 0, 0, 0 };
	const LoopEnd e = parse_blocks(
		c, 0, std::min<uint64_t>(c.blocks_promised(), max_blocks), nullptr, sink, MarkSink{ marks }, [&](uint64_t) { return block.data(); },
		[](uint64_t, const acmhip_blkhdr &) { return 0; });
	finish(info, e.b, e.status, sink.count);
	return ACM_OK;
}

bool acmstage::index_plausible(const acm_stage_info &info, size_t len, const acm_block_mark *marks, size_t blocks)
{
	if (!marks)
		return false;
	const uint64_t least = 20 + 5ull * info.cols;
	if (marks[0].bit < 8 * info.header_bytes)
		return false;
	for (size_t b = 0; b < blocks; b++)
		if (marks[b].bit >= 8ull * len || marks[b + 1].bit < marks[b].bit + least || marks[b].pwr > 15 || marks[b].val > 65535)
			return false;
	return marks[blocks].bit <= 8ull * len + 8;
}

int acmstage::stage_window(const uint8_t *data, size_t len, int force_chans, const acm_block_mark *marks, size_t nidx,
			   uint32_t block_first, uint32_t block_count, int16_t *idx, acmhip_blkhdr *hdr, std::vector<acmhip_patch> *patches,
			   acm_stage_info *info)
{
	memset(info, 0, sizeof(*info));
	Reader c;
	const int rc = c.open(data, len, force_chans);
	if (rc < 0)
		return rc;
	acmfill::fill_stage_info(&c.a, info);
	if (block_first > nidx)
		return ACMHIP_ERR_ARG;
	const size_t bl = c.a.block_len;
	const uint64_t want = std::min<uint64_t>(c.blocks_promised(), (uint64_t)block_first + block_count);

	/* Entering exactly at the end of the index means standing where the last indexed block left the reader - which may be in the
	 * zero byte behind the file.  That state is reached by parsing that block once more, into nothing. */
	uint64_t first = block_first;
	const bool via_last = block_first == nidx && nidx > 0 && first < want;
	if (via_last)
		first--;
	for (uint64_t k = 0; k < first; k++)
		c.tab.note_block(marks[k].pwr, marks[k].val);
	if (first > 0 && first < want && c.enter(marks[first].bit) < 0) {
		info->end_status = ACM_ERR_CORRUPT;
		return ACM_OK;
	}
	acmfill::PatchSink sink{ patches, 0, 0, 0 };
	std::vector<int16_t> dropped(via_last ? bl : 0);
	uint64_t staged = 0, count_before = 0;
	LoopEnd e = parse_blocks(
		c, first, want, nullptr, sink, MarkSink{ nullptr },
		[&](uint64_t b) {
			const bool keep = b >= block_first;
			sink.base_sample = staged * bl;
			sink.out = keep ? patches : nullptr;
			count_before = sink.count;
			return keep ? idx + staged * bl : dropped.data();
		},
		[&](uint64_t b, const acmhip_blkhdr &h) {
			const bool keep = b >= block_first;
			if (!keep)
				sink.count = count_before;
			/* the index says this block has this header and ends there: anything else is a stale or foreign index */
			if (b < nidx && (h.val != marks[b].val || h.pwr != marks[b].pwr || c.bit() != marks[b + 1].bit)) {
				if (keep && patches)
					patches->resize(patches->size() - (size_t)(sink.count - count_before));
				sink.count = count_before;
				return ACM_ERR_CORRUPT;
			}
			if (keep)
				hdr[staged++] = h;
			return 0;
		});
	if (e.status == 0 && e.b < want && e.b < nidx)
		e.status = ACM_ERR_CORRUPT;             /* ... and that it is whole, where the data ends in front of it or inside it */
	finish(info, staged, e.status, sink.count);
	return ACM_OK;
}

extern "C" int acm_stage_window(const uint8_t *data, size_t len, int force_chans, const acm_block_mark *marks, size_t nblocks_indexed,
				uint32_t block_first, uint32_t block_count, int16_t *idx, acmhip_blkhdr *hdr, acmhip_patch *patches,
				size_t max_patches, acm_stage_info *info)
{
	if (!data || !info || !marks || (block_count && (!idx || !hdr)) || (max_patches && !patches))
		return ACMHIP_ERR_ARG;
	acm_stage_info head;
	const int rc = acm_stage_probe(data, len, force_chans, &head);
	if (rc != ACM_OK) {
		memset(info, 0, sizeof(*info));
		return rc;
	}
	if (block_first > nblocks_indexed || !acmstage::index_plausible(head, len, marks, nblocks_indexed)) {
		memset(info, 0, sizeof(*info));
		return ACMHIP_ERR_ARG;
	}
	std::vector<acmhip_patch> found;
	const int r = acmstage::stage_window(data, len, force_chans, marks, nblocks_indexed, block_first, block_count, idx, hdr, &found, info);
	if (r != ACM_OK)
		return r;
	const size_t ncopy = std::min(found.size(), max_patches);
	if (ncopy)
		memcpy(patches, found.data(), ncopy * sizeof(acmhip_patch));
	return ACM_OK;
}

extern "C" int acmk_stage_marks(const uint8_t *data, size_t len, int force_chans, int stager, acm_block_mark *marks, size_t max_blocks,
				acm_stage_info *info)
{
	if (!data || !info || !marks || stager < 0 || stager > 2)
		return ACMHIP_ERR_ARG;
	int rc = acm_stage_probe(data, len, force_chans, info);
	if (rc != ACM_OK)
		return rc;
	const uint32_t level = info->level;
	const uint64_t bl = (uint64_t)info->rows * info->cols;
	if ((stager == 1 && acmhip_mform_tile_rows(level) <= 0) || (stager == 2 && acmhip_packed_tile_rows(level) <= 0))
		return ACMHIP_ERR_ARG;
	std::vector<int16_t> idx(std::max<uint64_t>(max_blocks * bl, 1));
	std::vector<acmhip_blkhdr> hdr(std::max<size_t>(max_blocks, 1));
	const uint64_t rows_cap = stager == 1 ? ((uint64_t)max_blocks * info->rows) & ~1ull : 0;
	std::vector<uint8_t> blob(rows_cap ? acmhip_mform_bytes(level, rows_cap) + 256 : 0);
	std::vector<acmhip_mform_pair> pairs(rows_cap ? acmhip_mform_pairs(rows_cap) + 32 : 0);
	const acmstage::MformArena mf{ blob.data(), 0, pairs.data() };
	acmstage::Staged st;
	rc = acmstage::stage_file(data, len, force_chans, idx.data(), hdr.data(), max_blocks, marks, rows_cap ? &mf : nullptr, &st);
	*info = st.info;
	if (rc == ACM_OK && stager == 2 && st.patches.empty()) {
		const uint64_t ntiles = (uint64_t)info->blocks * info->rows / (uint64_t)acmhip_packed_tile_rows(level);
		uint64_t bound = 0, bytes = 0;
		if (ntiles && acmhip_pack_bound(level, ntiles, &bound) == ACMHIP_OK) {
			std::vector<uint8_t> packed(bound);
			std::vector<acmhip_packed_chunk> chunks(ntiles * (uint64_t)acmhip_packed_slots(level));
			(void)acmhip_pack_tiles(level, idx.data(), ntiles, chunks.data(), packed.data(), 0, &bytes);
		}
	}
	return rc;
}
