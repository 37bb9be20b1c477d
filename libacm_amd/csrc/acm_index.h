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

namespace acmindex {

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

#endif
