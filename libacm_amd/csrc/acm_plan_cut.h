/*
 * acm_plan_cut.h - what a plan launches, decided on the host: the tables acm_hip_api.cpp uploads, as vectors.
 * Internal.  Neither this header nor acm_plan_cut.cpp knows a device: the cut depends on the descriptors, the
 * flags, the number of compute units and the acmk_* geometry queries alone (tests/test_plan_cut.py).
 */
#ifndef ACM_PLAN_CUT_H
#define ACM_PLAN_CUT_H

#include <vector>

#include "acm_device.h"

/* host twin of acm_hip_api.cpp's LevelGroup: vectors instead of device pointers */
struct AcmCutGroup {
	uint32_t level = 0;
	std::vector<AcmTile> tiles, tiles_extra;        /* `tiles` is the table the level launches: the lean kernels' rest, carry or halo flavour */
	bool carry = false;
	std::vector<AcmTile2> tiles2, tiles2p, tiles2p_plain, tiles2m, tiles2m_plain;
	std::vector<uint32_t> list;
	uint64_t max_elems = 0, max_emit = 0;
	bool prefix_patched = false;
	uint32_t prefix_stages = 0;
};

struct AcmPlanCut {
	std::vector<AcmDevStream> streams;              /* the n real ones, then the pseudo streams (patch windows, ragged tails, planes) */
	std::vector<AcmCutGroup> fused, small, prefix, stagewise;       /* each by rising level */
	std::vector<uint32_t> sw_all;                   /* every stage-wise stream, for the unpack launch */
	uint64_t sw_max_elems = 0, plane_elems = 0;
	std::vector<AcmDevPatch> patches;
	std::vector<uint64_t> form_rows;                /* per real stream: rows read from its second staged form */
	bool need_sink = false;                         /* a level launches a lean kernel: lead-in tiles need somewhere to store */
	int variant = 0;
	bool form_only = false;
	acmhip_plan_stats stats{};
};

/* ACMHIP_OK, or ACMHIP_ERR_ARG with the text left for acmhip_last_error(); `out` is a fresh AcmPlanCut */
int acm_plan_cut(int cus, const acmhip_stream_desc *streams, size_t n, const acmhip_packed_stream *packed,
		 const acmhip_patch *patches, size_t npatches, unsigned flags, AcmPlanCut *out);

extern "C" {
/* The cut shown to a visitor, table by table (tests): `visit` is called once per non-empty table with its name - streams, tiles,
 * tiles_extra, tiles2, tiles2p, tiles2p_plain, tiles2m, tiles2m_plain, small_list, prefix_list, prefix_tiles (the `tiles` of a prefix
 * group), sw_list, sw_all, patches, form_rows - and level (0 where there is none), then once with "stats": everything else a launch
 * depends on, as uint64 words - the acmhip_plan_stats, plane_elems, sw_max_elems, need_sink, the number of groups, and per group (fused,
 * small, prefix, stage-wise) its kind 0-3, level, carry, max_elems, max_emit, prefix_patched, prefix_stages.  Returns acm_plan_cut's
 * code; nothing is visited unless that is ACMHIP_OK */
typedef void (*acmk_cut_visit)(void *ctx, const char *table, uint32_t level, const void *data, size_t elem_bytes, size_t count);
int acmk_plan_cut_visit(int cus, const acmhip_stream_desc *streams, size_t n, const acmhip_packed_stream *packed,
			const acmhip_patch *patches, size_t npatches, unsigned flags, acmk_cut_visit visit, void *ctx);
}

#endif
