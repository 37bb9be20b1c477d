/*
 * acm_index.cpp - the block index of an ACM file, and host staging of a run of blocks entered through it (include/acm_hip.h).
 *
 * An ACM stream has no index of its own: where block b starts is known only once every block in front of it has been parsed
 * (decode.c:478-502).  But a block depends on the blocks in front of it in two ways only - where it starts, and what they left
 * in the never-cleared amplitude table (hazard H1, decode.c:809-810), which is a function of their (pwr, val) headers alone
 * (acmfill::TableHistory).  16 bytes per block - start bit, val, pwr - therefore let a reader enter the stream at any block and
 * produce exactly what a reader that came all the way from the header produces.  No device code here.
 */
#include "acm_index.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "acm_fill.h"
#include "libacm.h"

namespace {

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
	uint64_t bit() const { return acmindex::MarkSink::bit(a); }
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

uint64_t blocks_promised(const ACMStream &a)
{
	return ((uint64_t)a.total_values + a.block_len - 1) / a.block_len;
}

} // namespace

extern "C" int acm_index_file(const uint8_t *data, size_t len, int force_chans, acm_block_mark *marks, size_t max_blocks,
			      acm_stage_info *info)
{
	if (!data || !info || !marks)
		return ACMHIP_ERR_ARG;
	memset(info, 0, sizeof(*info));
	Reader c;
	int rc = c.open(data, len, force_chans);
	if (rc < 0)
		return rc;
	acmfill::fill_stage_info(&c.a, info);

	const uint64_t want = std::min<uint64_t>(blocks_promised(c.a), max_blocks);
	std::vector<int16_t> block(c.a.block_len);              /* the indices are parsed (H1 is counted) and dropped */
	acmfill::PatchSink sink{ nullptr, 0, 0, 0 };
	const acmindex::MarkSink mk{ marks };
	uint64_t b = 0;
	int status = 0;
	for (; b < want; b++) {
		acmhip_blkhdr h;
		mk.begin(b, c.a);
		rc = acmfill::parse_block(&c.a, &c.tab, block.data(), &h, &sink);
		if (rc != 1) {
			status = (rc == acmfill::kCleanEof) ? 0 : rc;
			break;
		}
		mk.whole(b, h);
	}
	mk.end(b, b == want, c.a);
	info->blocks = (uint32_t)b;
	info->end_status = status;
	info->npatches = sink.count;
	return ACM_OK;
}

bool acmindex::index_plausible(const acm_stage_info &info, size_t len, const acm_block_mark *marks, size_t blocks)
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

int acmindex::stage_window(const uint8_t *data, size_t len, int force_chans, const acm_block_mark *marks, size_t nidx,
			   uint32_t block_first, uint32_t block_count, int16_t *idx, acmhip_blkhdr *hdr, std::vector<acmhip_patch> *patches,
			   acm_stage_info *info)
{
	memset(info, 0, sizeof(*info));
	Reader c;
	int rc = c.open(data, len, force_chans);
	if (rc < 0)
		return rc;
	acmfill::fill_stage_info(&c.a, info);
	if (block_first > nidx)
		return ACMHIP_ERR_ARG;
	const size_t bl = c.a.block_len;
	const uint64_t want = std::min<uint64_t>(blocks_promised(c.a), (uint64_t)block_first + block_count);

	/* Entering exactly at the end of the index means standing where the last indexed block left the reader - which may be in the
	 * zero byte behind the file.  That state is reached by parsing that block once more, into nothing. */
	uint64_t b = block_first;
	const bool via_last = block_first == nidx && nidx > 0 && b < want;
	if (via_last)
		b--;
	for (uint64_t k = 0; k < b; k++)
		c.tab.note_block(marks[k].pwr, marks[k].val);
	if (b > 0 && b < want) {
		rc = c.enter(marks[b].bit);
		if (rc < 0) {
			info->end_status = ACM_ERR_CORRUPT;
			return ACM_OK;
		}
	}
	acmfill::PatchSink sink{ patches, 0, 0, 0 };
	std::vector<int16_t> dropped(via_last ? bl : 0);
	uint64_t staged = 0;
	int status = 0;
	for (; b < want; b++) {
		const bool keep = b >= block_first;
		acmhip_blkhdr h;
		sink.base_sample = staged * bl;
		if (!keep)
			sink.out = nullptr;
		const uint64_t count_before = sink.count;
		rc = acmfill::parse_block(&c.a, &c.tab, keep ? idx + staged * bl : dropped.data(), &h, &sink);
		if (!keep) {
			sink.out = patches;
			sink.count = count_before;
		}
		if (b < nidx) {
			/* the index says this block is whole, has this header and ends there: anything else is a stale or foreign index */
			if (rc == acmfill::kCleanEof || (rc == 1 && (h.val != marks[b].val || h.pwr != marks[b].pwr || c.bit() != marks[b + 1].bit))) {
				if (rc == 1 && keep && patches)
					patches->resize(patches->size() - (size_t)(sink.count - count_before));
				if (rc == 1 && keep)
					sink.count = count_before;
				status = ACM_ERR_CORRUPT;
				break;
			}
		}
		if (rc != 1) {
			status = (rc == acmfill::kCleanEof) ? 0 : rc;
			break;
		}
		if (keep)
			hdr[staged++] = h;
	}
	info->blocks = (uint32_t)staged;
	info->end_status = status;
	info->npatches = sink.count;
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
	if (block_first > nblocks_indexed || !acmindex::index_plausible(head, len, marks, nblocks_indexed)) {
		memset(info, 0, sizeof(*info));
		return ACMHIP_ERR_ARG;
	}
	std::vector<acmhip_patch> found;
	const int r = acmindex::stage_window(data, len, force_chans, marks, nblocks_indexed, block_first, block_count, idx, hdr, &found, info);
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
	std::vector<int16_t> idx(std::max<uint64_t>(max_blocks * bl, 1));
	std::vector<acmhip_blkhdr> hdr(std::max<size_t>(max_blocks, 1));
	if (stager == 1) {
		if (acmhip_mform_tile_rows(level) <= 0)
			return ACMHIP_ERR_ARG;
		const uint64_t rows_cap = ((uint64_t)max_blocks * info->rows) & ~1ull;
		std::vector<uint8_t> mf(acmhip_mform_bytes(level, rows_cap) + 256);
		std::vector<acmhip_mform_pair> pairs(acmhip_mform_pairs(rows_cap) + 32);
		uint64_t mf_rows = 0, mf_bytes = 0;
		rc = rows_cap ? acmindex::stage_file_mform(data, len, force_chans, idx.data(), hdr.data(), max_blocks, info, mf.data(), 0, pairs.data(), &mf_rows,
							   &mf_bytes, marks)
			      : acmindex::stage_file(data, len, force_chans, idx.data(), hdr.data(), max_blocks, nullptr, 0, info, marks);
	} else {
		if (stager == 2 && acmhip_packed_tile_rows(level) <= 0)
			return ACMHIP_ERR_ARG;
		rc = acmindex::stage_file(data, len, force_chans, idx.data(), hdr.data(), max_blocks, nullptr, 0, info, marks);
	}
	if (rc == ACM_OK && info->npatches) {
		std::vector<acmhip_patch> patches(info->npatches);
		rc = acmindex::stage_file(data, len, force_chans, idx.data(), hdr.data(), max_blocks, patches.data(), patches.size(), info, nullptr);
	}
	if (rc == ACM_OK && stager == 2 && !info->npatches) {
		const uint64_t ntiles = (uint64_t)info->blocks * info->rows / (uint64_t)acmhip_packed_tile_rows(level);
		uint64_t bound = 0, bytes = 0;
		if (ntiles && acmhip_pack_bound(level, ntiles, &bound) == ACMHIP_OK) {
			std::vector<uint8_t> blob(bound);
			std::vector<acmhip_packed_chunk> chunks(ntiles * (uint64_t)acmhip_packed_slots(level));
			(void)acmhip_pack_tiles(level, idx.data(), ntiles, chunks.data(), blob.data(), 0, &bytes);
		}
	}
	return rc;
}
