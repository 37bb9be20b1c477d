/*
 * acm_stage.h - the host stagers of a file image held in memory (acm_stage.cpp): the block index, whole files as int16 rows or in the
 * byte-plane form, and a run of blocks entered through the index.  Internal; the public calls are acm_stage_probe / acm_stage_file /
 * acm_stage_file_mform / acm_index_file / acm_stage_window of include/acm_hip.h.  No device code behind this header.
 */
#ifndef ACM_STAGE_H
#define ACM_STAGE_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "acm_hip.h"
#include "libacm.h"

namespace acmstage {

/* The index as a by-product of a reader's block loop: acm_index_file's rule for a block that fails and for the entry behind the last
 * one, stated once for acm_index_file and for the stagers that hand the index out beside what they stage.  marks may be null: nothing
 * is kept.  The loop calls begin() where it stands in front of block b, whole() once parse_block has returned 1 for it, and end() with
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

/* what staging a file yields besides the rows, headers and marks in the caller's buffers */
struct Staged {
	acm_stage_info info{};
	std::vector<acmhip_patch> patches;      /* every H1 patch of the staged blocks, in stream order */
	uint64_t mf_rows = 0, mf_bytes = 0;     /* rows [0, mf_rows) are in the byte-plane form, in mf_bytes of the blob; 0: none */
};

/* a byte-plane arena offered to stage_file: acm_stage_file_mform's mf_out, mf_base and pairs */
struct MformArena {
	uint8_t *out;
	uint64_t base;
	acmhip_mform_pair *pairs;
};

/* acm_stage_file - or, with an arena, acm_stage_file_mform - in ONE call whatever the stream holds: every patch comes back in
 * out->patches, so no caller stages a file a second time to make room for them.  marks (may be null) has room for max_blocks + 1
 * entries and receives what acm_index_file(data, len, force_chans, marks, max_blocks, ..) writes.  A stream that cannot have the form
 * (acm_stage_file_mform names the cases) is staged the plain way and out->mf_rows is 0 */
int stage_file(const uint8_t *data, size_t len, int force_chans, int16_t *idx, acmhip_blkhdr *hdr, size_t max_blocks, acm_block_mark *marks,
	       const MformArena *mf, Staged *out);

/* Is marks[0 .. blocks] an index a file of `len` bytes with this header can have?  Bits behind the header, strictly increasing,
 * every block at least its 20-bit header and a 5-bit code per column long, the indexed blocks inside the file (the end entry may
 * lie in the one zero byte the reader appends, decode.c:57-61).  Says nothing about the CONTENTS of the file: that is checked
 * block by block while staging. */
bool index_plausible(const acm_stage_info &info, size_t len, const acm_block_mark *marks, size_t blocks);

/* acm_stage_window without the index check and with the patches in a vector (may be null: count only) */
int stage_window(const uint8_t *data, size_t len, int force_chans, const acm_block_mark *marks, size_t nblocks_indexed,
		 uint32_t block_first, uint32_t block_count, int16_t *idx, acmhip_blkhdr *hdr, std::vector<acmhip_patch> *patches,
		 acm_stage_info *info);

} // namespace acmstage

extern "C" {
/* Test hook, no device: one file through acmstage::stage_file the way a batch's pool calls it for `stager` - 0 int16 rows, 1 with a
 * byte-plane arena, 2 int16 rows + acmhip_pack_tiles (the packed form); what is staged is dropped, only the return code, *info and
 * marks[0 .. max_blocks] come back.  ACMHIP_ERR_ARG for a level that does not have the form asked for */
int acmk_stage_marks(const uint8_t *data, size_t len, int force_chans, int stager, acm_block_mark *marks, size_t max_blocks, acm_stage_info *info);
}

#endif
