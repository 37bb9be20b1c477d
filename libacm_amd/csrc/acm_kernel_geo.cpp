/*
 * acm_kernel_geo.cpp - every acmk_* query that launches nothing, answered from the tables of acm_kernel_geo.h: what the planner
 * (acm_plan_cut.cpp), the layouts, the stagers (acm_stage.cpp, acm_pack.cpp) and the launchers themselves ask about a kernel build.
 * Plain C++: no device, no HIP header, no kernel - the sanitizer harnesses under tests/native link it as it is.
 * Also here, because they are decisions and not kernels: which build of a level a process uses (tile2m_at), how a launch of the
 * chunk kernel shares its table (acmk_tile2m_split), and what the device parser accepts and where its stripes and ranges are cut.
 */
#include <stdlib.h>

#include "acm_kernel_geo.h"
#include "acm_parse_bounds.h"

using namespace acm_geo;

namespace {

inline int cus_of(int cus) { return cus > 0 ? cus : 256; }
inline int switch_of(const char *text, int unset) { return text ? atoi(text) : unset; }

inline const FusedTile *fused_at(uint32_t level, int variant)
{
	if (level < ACM_K1_MIN_LEVEL || level > ACM_K1_MAX_LEVEL || variant < 0 || variant >= NVARIANTS)
		return nullptr;
	return &FUSED[variant][level - ACM_K1_MIN_LEVEL];
}

/* the byte-plane build a level uses in this process (null: the level has none) */
const Tile2MTile *tile2m_at(uint32_t level, int *g0 = nullptr)
{
	if (level < ACM_K2M_MIN_LEVEL || level > ACM_K2M_MAX_LEVEL)
		return nullptr;
	/* (tuning builds: ACM_K3=0 puts levels 8-12 back on acm_tile2's three / four-stage matrix build - and on ITS form: process-wide,
	 * read once, because the staged form follows the kernel, acmhip_mform_group) */
	static const bool k3 = switch_of(ACM_TUNING_ENV("ACM_K3"), 1) != 0;
	static const int forced = switch_of(ACM_TUNING_ENV("ACM_K2M_G0"), 0);
	const Tile2MTile *row = TILE2M[level - ACM_K2M_MIN_LEVEL];
	const int want = forced ? forced : TILE2M_DEFAULT_G0[level - ACM_K2M_MIN_LEVEL];
	const int slot = k3 && row[2].t.nt ? 2 : (want == 4 || !row[0].t.nt) && row[1].t.nt ? 1 : 0;
	if (g0)
		*g0 = row[slot].t.nt ? TILE2M_G0[slot] : 0;
	return &row[slot];
}

inline const PackTile *tile2p_at(uint32_t level)
{
	return level < ACM_K2P_MIN_LEVEL || level > ACM_K2P_MAX_LEVEL ? nullptr : &TILE2P[level - ACM_K2P_MIN_LEVEL];
}

} // namespace

extern "C" uint64_t acmk_geo_digest(void)
{
	return digest();
}

extern "C" int acmk_tuning_build(void)
{
#ifdef ACM_TUNING
	return 1;
#else
	return 0;
#endif
}

// ---------------------------------------------------------------------------
// acm_fused_tile and its plane build
// ---------------------------------------------------------------------------
extern "C" int acmk_fused_variants(void)
{
	return NVARIANTS;
}

extern "C" int acmk_fused_tile_rows(uint32_t level, int variant)
{
	const FusedTile *f = fused_at(level, variant);
	return f ? fused_launch(*f, (int)level).tile_rows : 0;
}

extern "C" int acmk_fused_has_carry(uint32_t level, int variant)
{
	const FusedTile *f = fused_at(level, variant);
	return f && f->carry;
}

extern "C" int acmk_fused_threads(uint32_t level, int variant)
{
	const FusedTile *f = fused_at(level, variant);
	return f ? f->t.nt : 0;
}

/* persistent grid: as many workgroups as the chip holds at once.  `cus` comes from the device handle: nothing here queries or
 * synchronises, so a launch can be captured into a hipGraph */
extern "C" int acmk_fused_grid(uint32_t level, int variant, int cus)
{
	const FusedTile *f = fused_at(level, variant);
	return f ? cus_of(cus) * fused_launch(*f, (int)level).wg_per_cu : 0;
}

extern "C" int acmk_plane_tile_rows(void)
{
	return fused_launch(PLANE, 12).tile_rows;
}

extern "C" int acmk_plane_threads(void)
{
	return PLANE.t.nt;
}

extern "C" int acmk_plane_grid(int cus)
{
	return cus_of(cus) * fused_launch(PLANE, 12).wg_per_cu;
}

// ---------------------------------------------------------------------------
// acm_tile2
// ---------------------------------------------------------------------------
extern "C" int acmk_tile2_rows(uint32_t level)
{
	if (level < ACM_K2_MIN_LEVEL || level > ACM_K2_MAX_LEVEL)
		return 0;
	return launch_of(TILE2[level - ACM_K2_MIN_LEVEL], (int)level).tile_rows;
}

extern "C" int acmk_tile2_threads(uint32_t level)
{
	if (level < ACM_K2_MIN_LEVEL || level > ACM_K2_MAX_LEVEL)
		return 0;
	return TILE2[level - ACM_K2_MIN_LEVEL].nt;
}

extern "C" int acmk_tile2_grid(uint32_t level, int cus)
{
	if (level < ACM_K2_MIN_LEVEL || level > ACM_K2_MAX_LEVEL)
		return 0;
	return cus_of(cus) * TILE2[level - ACM_K2_MIN_LEVEL].w;
}

// ---------------------------------------------------------------------------
// the byte-plane builds: acm_tile2 with the first pass on the matrix cores, acm_chunk
// ---------------------------------------------------------------------------
extern "C" int acmk_tile2m_rows(uint32_t level)
{
	const Tile2MTile *m = tile2m_at(level);
	return m ? launch_of(m->t, (int)level).tile_rows : 0;
}

extern "C" int acmk_tile2m_threads(uint32_t level)
{
	const Tile2MTile *m = tile2m_at(level);
	return m ? m->t.nt : 0;
}

/* stages of the first pass of the build the level uses: which build that is (3, 4: acm_tile2's matrix builds; 6: acm_chunk, or
 * FirstPassZW inside acm_tile2 at levels 13 and 14).  acmk_launch_tile2m picks its kernel by this answer */
extern "C" int acmk_tile2m_stages(uint32_t level)
{
	int g0 = 0;
	return tile2m_at(level, &g0) ? g0 : 0;
}

/* tiles of this build the planner puts in front of a window into a stream (acm_kernel_geo.h: lead_in_of) */
extern "C" int acmk_tile2m_lead_in(uint32_t level)
{
	const Tile2MTile *m = tile2m_at(level);
	return m && m->t.nt ? m->lead_in : 1;
}

/* wavefronts that share a launch of the chunk kernel's table among them (each takes one contiguous run of it); 0: not the chunk kernel */
extern "C" int acmk_tile2m_run_waves(uint32_t level, int cus)
{
	const Tile2MTile *m = tile2m_at(level);
	return m && m->chunk ? cus_of(cus) * m->t.w * (m->t.nt / 64) : 0;
}

/* workgroups of a launch of the byte-plane build at most (the same as acmk_tile2_grid except at level 13, whose tiles are half as tall) */
extern "C" int acmk_tile2m_grid(uint32_t level, int cus)
{
	const Tile2MTile *m = tile2m_at(level);
	return m ? cus_of(cus) * m->t.w : 0;
}

/* How a launch of the chunk kernel hands its table of ntiles chunks to the W = acmk_tile2m_run_waves wavefronts (device-free: the launcher
 * and the tests call it).  The first W * static_per chunks are static runs, wavefront w's the chunks [w * static_per, (w + 1) *
 * static_per); the rest is cut into nclaimed runs of run_chunks (the last one may be shorter), run k at chunk W * static_per + k *
 * run_chunks, which the wavefronts claim in ascending k as they come free.
 * The rule: under the compiled-in policy of the level (g_claim_default: run_chunks - 0: the level keeps the static split - and the static
 * share in thousandths of the table) a table is split this way from ACM_CLAIM_MIN_PER chunks per wavefront on; a policy set through
 * acmk_tile2m_claim_config holds for every table of at least as many chunks as a launch has workgroups at most.  Either way static_per =
 * floor(ntiles * share / 1000 / W), and a table that leaves nothing behind its static runs is not split.
 * Every other table stays wholly static exactly as before: nclaimed = 0, run_chunks = 0, static_per = ceil(ntiles / W), one contiguous
 * run per wavefront.  Returns 0, or -1 for a level without the chunk kernel */
#define ACM_CLAIM_MIN_PER 32u
#ifndef ACM_CLAIM_DEFAULTS
#define ACM_CLAIM_DEFAULTS { 16, 900 }, { 16, 800 }, { 16, 800 }, { 16, 800 }, { 16, 900 }
#endif
/* (levels 8-12, measured on 1024 streams of 2 Mi samples, profiles/claimed_runs_notes.txt 2: the oldest wavefront of a SIMD is done
 * with an equal share at 0.8 of the launch, so a fifth of the table is what there is to hand out; runs of 8 replay too many chunks, runs
 * of 32 and more leave too long a tail) */
static const struct { int run_chunks, static_permille; } g_claim_default[5] = { ACM_CLAIM_DEFAULTS };
static int g_claim_run_chunks = -1, g_claim_static_permille = -1;         /* < 0: the level's default */

extern "C" int acmk_tile2m_split(uint32_t level, int cus, uint32_t ntiles, uint32_t *static_per, uint32_t *run_chunks, uint32_t *nclaimed)
{
	const uint32_t W = (uint32_t)acmk_tile2m_run_waves(level, cus);
	if (!W)
		return -1;
	const bool set = g_claim_run_chunks >= 0 || g_claim_static_permille >= 0;
	const uint32_t R = (uint32_t)(g_claim_run_chunks >= 0 ? g_claim_run_chunks : g_claim_default[level - 8].run_chunks);
	uint32_t share = (uint32_t)(g_claim_static_permille >= 0 ? g_claim_static_permille : g_claim_default[level - 8].static_permille);
	if (share > 1000u)
		share = 1000u;
	*static_per = (ntiles + W - 1) / W;
	*run_chunks = *nclaimed = 0;
	if (!R || ntiles < (set ? (uint32_t)acmk_tile2m_grid(level, cus) : W * ACM_CLAIM_MIN_PER))
		return 0;
	const uint32_t sp = (uint32_t)((uint64_t)ntiles * share / 1000u / W);
	const uint32_t rest = ntiles - W * sp;
	if (!rest)
		return 0;
	*static_per = sp;
	*run_chunks = R;
	*nclaimed = (rest + R - 1) / R;
	return 0;
}

/* process-wide policy for every level, for tests and sweeps: run_chunks (0: no claimed runs) and the static share in thousandths; a
 * negative argument puts that value back to the levels' defaults.  Hands back what was set before (negative: the defaults) */
extern "C" void acmk_tile2m_claim_config(int run_chunks, int static_permille, int *old_run_chunks, int *old_static_permille)
{
	if (old_run_chunks)
		*old_run_chunks = g_claim_run_chunks;
	if (old_static_permille)
		*old_static_permille = g_claim_static_permille;
	g_claim_run_chunks = run_chunks < 0 ? -1 : run_chunks;
	g_claim_static_permille = static_permille < 0 ? -1 : static_permille;
}

// ---------------------------------------------------------------------------
// acm_tile2p
// ---------------------------------------------------------------------------
extern "C" int acmk_tile2p_rows(uint32_t level)
{
	const PackTile *p = tile2p_at(level);
	return p ? launch_of(p->t, (int)level).tile_rows : 0;
}

extern "C" int acmk_tile2p_group_rows(uint32_t level)
{
	const PackTile *p = tile2p_at(level);
	return p ? p->gr : 0;
}

extern "C" int acmk_tile2p_slots(uint32_t level)
{
	return tile2p_at(level) ? TILE2P_SLOTS[level - ACM_K2P_MIN_LEVEL].slots : 0;
}

extern "C" int acmk_tile2p_waves(uint32_t level)
{
	const PackTile *p = tile2p_at(level);
	return p ? p->t.nt / 64 : 0;
}

extern "C" int acmk_tile2p_pad_shift(uint32_t level)
{
	return tile2p_at(level) ? TILE2P_SLOTS[level - ACM_K2P_MIN_LEVEL].pad_shift : 0;
}

extern "C" int acmk_tile2p_grid(uint32_t level, int cus)
{
	const PackTile *p = tile2p_at(level);
	return p ? cus_of(cus) * p->t.w : 0;
}

// ---------------------------------------------------------------------------
// the device parser
// ---------------------------------------------------------------------------
extern "C" int acmk_parse_supported(uint32_t level, uint32_t rows, uint64_t file_len, uint64_t blocks)
{
	/* 32-bit bit offsets with headroom (a corrupt stream may step one column past the end of its file before
	 * the walk notices, and must not wrap), 32-bit column counts */
	return rows >= 1 && blocks >= 1 && file_len < 0x10000000ull && (blocks << level) < 0xFFFFFFFFull;
}

extern "C" uint32_t acmk_stripe_bound(uint32_t file_len, uint32_t s, uint32_t S)
{
	return acm_stripe_bound(file_len, s, S);
}

extern "C" uint32_t acmk_range_bound(uint32_t blocks, uint32_t r, uint32_t R, uint32_t unit)
{
	return acm_range_bound(blocks, r, R, unit);
}

// ---------------------------------------------------------------------------
// launch caps (acmhip_device_set_launch_caps): the check and the exchange, without a device
// ---------------------------------------------------------------------------
extern "C" int acmk_launch_caps_set(acmhip_launch_caps *held, const acmhip_launch_caps *caps, acmhip_launch_caps *previous)
{
	if (!held)
		return ACMHIP_ERR_ARG;
	const acmhip_launch_caps none{};
	const acmhip_launch_caps &c = caps ? *caps : none;
	if (c.list_slice > ACM_CAP_LIST_SLICE || c.small_grid_x > ACM_CAP_SMALL_GRID_X || c.parse_slice > ACM_CAP_PARSE_SLICE ||
	    c.parse_grid_x > ACM_CAP_PARSE_GRID_X || c.dense_grid > ACM_CAP_DENSE_GRID)
		return ACMHIP_ERR_ARG;
	const acmhip_launch_caps was = *held;           /* (previous may be caps itself, or held) */
	*held = c;
	if (previous)
		*previous = was;
	return ACMHIP_OK;
}
