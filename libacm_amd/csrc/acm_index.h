/*
 * acm_index.h - the block index of a file and the host stager that enters a stream through it (acm_index.cpp).
 * Internal; the public calls are acm_index_file / acm_stage_window of include/acm_hip.h.
 */
#ifndef ACM_INDEX_H
#define ACM_INDEX_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "acm_hip.h"
#include "libacm.h"

namespace acmindex {

/* The index as a by-product of a reader's block loop: acm_index_file's rule for a block that fails and for the entry behind the last
 * one, stated once for acm_index_file and for the stagers that hand the index out beside what they stage.  marks may be null: nothing
 * is kept.  A loop calls begin() where it stands in front of block b, whole() once parse_block has returned 1 for it, and end() with
 * the number of whole blocks when it is over */
struct MarkSink {
	acm_block_mark *marks;
	/* file bit offset of the reader's next unread bit (the buffer starts at file byte buf_start_ofs: the source is read in order) */
	static uint64_t bit(const ACMStream &a) { return 8ull * ((uint64_t)a.buf_start_ofs + a.buf_pos) - a.bit_avail; }
	void begin(uint64_t b, const ACMStream &a) const
	{
		if (marks)
			marks[b].bit = bit(a);
	}
	void whole(uint64_t b, const acmhip_blkhdr &h) const
	{
		if (marks) {
			marks[b].val = h.val;
			marks[b].pwr = h.pwr;
		}
	}
	/* `all`: every block asked for is whole, the entry behind them is where the reader stands.  Else block b failed and its start - the
	 * bit behind the last whole one, written by begin() - stays */
	void end(uint64_t b, bool all, const ACMStream &a) const
	{
		if (!marks)
			return;
		if (all)
			marks[b].bit = bit(a);
		marks[b].val = marks[b].pwr = 0;
	}
};

/* acm_stage_file / acm_stage_file_mform (acm_stream.cpp) with the index of what they stage as a by-product: marks (may be null) has room
 * for max_blocks + 1 entries and receives what acm_index_file(data, len, force_chans, marks, max_blocks, ..) writes */
int stage_file(const uint8_t *data, size_t len, int force_chans, int16_t *idx, acmhip_blkhdr *hdr, size_t max_blocks, acmhip_patch *patches,
	       size_t max_patches, acm_stage_info *info, acm_block_mark *marks);
int stage_file_mform(const uint8_t *data, size_t len, int force_chans, int16_t *idx, acmhip_blkhdr *hdr, size_t max_blocks, acm_stage_info *info,
		     uint8_t *mf_out, uint64_t mf_base, acmhip_mform_pair *pairs, uint64_t *mf_rows, uint64_t *mf_bytes, acm_block_mark *marks);

/* Is marks[0 .. blocks] an index a file of `len` bytes with this header can have?  Bits behind the header, strictly increasing,
 * every block at least its 20-bit header and a 5-bit code per column long, the indexed blocks inside the file (the end entry may
 * lie in the one zero byte the reader appends, decode.c:57-61).  Says nothing about the CONTENTS of the file: that is checked
 * block by block while staging. */
bool index_plausible(const acm_stage_info &info, size_t len, const acm_block_mark *marks, size_t blocks);

/* acm_stage_window without the index check and with the patches in a vector (may be null: count only) */
int stage_window(const uint8_t *data, size_t len, int force_chans, const acm_block_mark *marks, size_t nblocks_indexed,
		 uint32_t block_first, uint32_t block_count, int16_t *idx, acmhip_blkhdr *hdr, std::vector<acmhip_patch> *patches,
		 acm_stage_info *info);

} // namespace acmindex

extern "C" {
/* Test hook, no device: one file through the host stager a batch's pool picks for `stager` - 0 acm_stage_file (int16 rows), 1
 * acm_stage_file_mform (the byte-plane form), 2 acm_stage_file + acmhip_pack_tiles (the packed form) - with a second pass for H1 patches
 * as the pool makes it; what is staged is dropped, only the return code, *info and marks[0 .. max_blocks] come back.  ACMHIP_ERR_ARG for
 * a level that does not have the form asked for */
int acmk_stage_marks(const uint8_t *data, size_t len, int force_chans, int stager, acm_block_mark *marks, size_t max_blocks, acm_stage_info *info);
}

#endif
