/*
 * acm_plan_cut.cpp - the launch planner's host half: which kernel family decodes which rows of which stream.
 * Plain C++ over vectors, no device involved; the plan-creation calls upload what acm_plan_cut() returns.
 */
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "acm_plan_cut.h"

#define ACM_K1_DEFAULT_VARIANT 0
/* AcmTile2.hdr_blk is 32 bits wide, and the byte-plane kernels index the pair table in 32 bits (and fetch whole groups of entries: the
 * table's 32 entries of read slack): header and pair-table indices end below 2^32 (include/acm_hip.h: hdr_off, chunk_off) */
#define ACM_TABLE_INDEX_END (1ull << 32)
#define ACM_PAIR_READ_SLACK 32u

namespace {

void set_err(const char *fmt, ...)
{
	char text[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(text, sizeof(text), fmt, ap);
	va_end(ap);
	acmhip_set_error_text(text);
}

bool fused_ok(const acmhip_stream_desc &s, int variant)
{
	return s.level >= ACM_K1_MIN_LEVEL && s.level <= ACM_K1_MAX_LEVEL && acmk_fused_tile_rows(s.level, variant) > 2;
}

/* Default: carry mode saves 2 of every tile_rows rows and costs one lead-in tile per workgroup, so it pays from tile_rows/2 tiles per
 * workgroup on; it is taken from tile_rows tiles per workgroup.  ACMHIP_PLAN_FORCE_HALO / _CARRY force a flavour (tests, measurements) */
bool carry_wanted(size_t ntiles, size_t grid, size_t tile_rows, unsigned flags)
{
	if (flags & (ACMHIP_PLAN_FORCE_HALO | ACMHIP_PLAN_FORCE_CARRY))
		return (flags & ACMHIP_PLAN_FORCE_CARRY) != 0;
	if (const char *e = ACM_TUNING_ENV("ACM_K1_CARRY"))
		return atoi(e) != 0;
	return grid > 0 && ntiles >= tile_rows * grid;
}

/* the lean kernels: -1 by tile count (default), 0 never (ACMHIP_PLAN_NO_LEAN), 1 whenever there is a whole tile (ACMHIP_PLAN_LEAN_ALWAYS) */
int lean_policy(unsigned flags)
{
	if (flags & ACMHIP_PLAN_NO_LEAN)
		return 0;
	if (flags & ACMHIP_PLAN_LEAN_ALWAYS)
		return 1;
	if (const char *e = ACM_TUNING_ENV("ACM_K2"))
		return atoi(e) != 0;
	return -1;
}

/* levels 13-15 on the prefix + plane pair (default), or on the stage-wise kernels like any level without a kernel of its own */
bool prefix_policy(unsigned flags)
{
	const char *e = ACM_TUNING_ENV("ACM_PREFIX");
	return !(flags & ACMHIP_PLAN_STAGEWISE) && !(e && atoi(e) == 0);
}

/* tuning builds: ACM_K1_VARIANT=n picks another built-in tile geometry (default: the measured-best one) */
int pick_variant()
{
	int v = ACM_K1_DEFAULT_VARIANT;
	if (const char *e = ACM_TUNING_ENV("ACM_K1_VARIANT"))
		v = atoi(e);
	if (v < 0 || v >= acmk_fused_variants())
		v = ACM_K1_DEFAULT_VARIANT;
	return v;
}

bool valid_desc(const acmhip_stream_desc &s)
{
	return !(s.level > 15 || s.rows == 0 || s.rows > 4095 || (s.idx_off & 7) || (s.pcm_off & 7) || s.row_begin > s.nrows ||
		 s.n_emit > ((uint64_t)(s.nrows - s.row_begin) << s.level));
}

AcmDevStream dev_stream_of(const acmhip_stream_desc &s)
{
	AcmDevStream d{};
	d.idx_off = s.idx_off;
	d.hdr_off = s.hdr_off;
	d.pcm_off = s.pcm_off;
	d.n_emit = s.n_emit;
	d.level = s.level;
	d.rows = s.rows;
	d.nrows = s.nrows;
	d.row_begin = s.row_begin;
	d.halo_row = s.row_begin >= 2 ? s.row_begin - 2 : 0;
	return d;
}

/* (room for a stream's records in one step - doubling, or every stream would move the whole table) */
void room(std::vector<AcmTile2> &v, uint64_t more)
{
	if (v.capacity() < v.size() + more)
		v.reserve(std::max<size_t>(2 * v.capacity(), v.size() + more));
}

/* The carry-mode table of a stream whose emit_rows rows from row_begin on are cut into tiles of TC payload rows: a stream that does not
 * start at its row 0 gets a lead-in tile in front (rows that do not exist count as zeros, which is exact: no output depends on anything
 * further back than two rows) */
void cut_carry(std::vector<AcmTile> &tc, uint32_t id, uint32_t row_begin, uint64_t emit_rows, uint32_t TC)
{
	if (row_begin > 0)
		tc.push_back(AcmTile{ id, (int32_t)row_begin - (int32_t)TC, ACM_TILE_FRESH | ACM_TILE_DISCARD, 0u });
	for (uint64_t r = 0; r < emit_rows; r += TC)
		tc.push_back(AcmTile{ id, (int32_t)(row_begin + r), (r == 0 && row_begin == 0) ? ACM_TILE_FRESH : 0u, 0u });
}

/* rows [row0, ...) of a stream on the lean kernels: what its records of every build share */
struct LeanRows {
	const acmhip_stream_desc &s;
	uint64_t row0;
	uint32_t magic;         /* ceil(2^32 / rows): AcmTile2 */

	/* (a lead-in that is the stream's first tile has nothing in front of it either: both flags) */
	uint32_t flags_of(uint64_t r, bool lead_in) const { return (lead_in ? ACM_TILE_DISCARD : 0u) | (r == 0 ? ACM_TILE_FRESH : 0u); }
	/* where sample (row r, column 0) goes: rows count from the window's first row (a lead-in stores into the sink) */
	uint64_t pcm_of(uint64_t r) const { return s.pcm_off + ((r >= row0 ? r - row0 : 0) << s.level); }
};

/* The byte-plane records of the tile [r, r + T2): chunks of T2M rows.  A byte-plane tile is named by the pair-table entry of the row pair
 * in front of it (entry 0 of a stream: the pair of zeros).  Chunks of one row - T2M == 1, the chunk kernel at levels 11 and 12 - also say
 * whether they start a pair and whether they are row 1; of a lead-in tile only the last chunks are needed, lead_rows rows of them */
void cut_chunks(std::vector<AcmTile2> &mtab, const LeanRows &w, uint64_t chunk_off, uint64_t r, bool lead_in, uint32_t T2, uint32_t T2M,
		uint64_t lead_rows)
{
	const uint32_t srows = w.s.rows;
	uint64_t rm = lead_in ? r + T2 - std::min<uint64_t>(T2, lead_rows) : r;
	const uint32_t rhm0 = (uint32_t)(rm >= 2 ? rm - 2 : 0);
	uint32_t blk = rhm0 / srows, pos = rhm0 % srows;        /* of row rm - 2, carried along from chunk to chunk */
	for (; rm < r + T2; rm += T2M) {
		/* rows in reach: max(rm - 2, 0) - the row (blk, pos) names - through rm + T2M - 1 */
		const uint64_t span = rm + T2M - 1 - (rm >= 2 ? rm - 2 : 0);
		mtab.push_back(AcmTile2{ chunk_off + rm / 2, w.pcm_of(rm), (uint32_t)w.s.hdr_off + blk, pos, w.magic,
					 w.flags_of(rm, lead_in) | (rm == 1 ? ACM_TILE_ROW1 : 0u) | ((rm & 1) ? ACM_TILE_ODD : 0u) |
					 (pos + span < srows ? ACM_TILE_ONEBLOCK : 0u) });
		/* the next chunk's row rm + T2M - 2 (rows 0 and 1 of a stream both count from row 0) */
		const uint32_t step = rm >= 2 ? T2M : rm + T2M >= 2 ? (uint32_t)(rm + T2M - 2) : 0u;
		pos += step;
		while (pos >= srows) {
			pos -= srows;
			blk++;
		}
	}
}

/* everything the cut keeps per level while the streams are walked */
struct LevelCut {
	std::vector<AcmTile> tiles, tiles_carry, tiles_rest, tiles_extra;       /* fused kernel: halo flavour, carry flavour, what the lean kernels leave, clean tiles of patched streams */
	std::vector<AcmTile2> tiles2, tiles2p, tiles2p_plain, tiles2m, tiles2m_plain;
	std::vector<AcmTile> prefix_tiles, prefix_tiles_carry;                  /* levels 13-15: the plane kernel's tiles */
	std::vector<uint32_t> list, small_list, prefix_list;
	uint64_t max_elems = 0, max_emit = 0;
	bool k2_high = false;           /* levels 13, 14: the batch has enough whole tiles for the lean kernel */
};

/* H1 patches (stale amplitude table): only the tiles that can see a patched sample leave the tile kernel - each of them
 * becomes a window of its stream for the stage-wise kernels (a pseudo stream behind the n real ones) */
struct PatchWindow {
	uint32_t stream;
	uint64_t lo_row, hi_row, scratch_off;
};

struct Cutter {
	const int cus;
	const acmhip_stream_desc *const streams;
	const size_t n;
	const acmhip_packed_stream *const packed;
	const acmhip_patch *const patches;
	const size_t npatches;
	const unsigned flags;
	AcmPlanCut &cut;
	Cutter(int cus_, const acmhip_stream_desc *streams_, size_t n_, const acmhip_packed_stream *packed_, const acmhip_patch *patches_,
	       size_t npatches_, unsigned flags_, AcmPlanCut &cut_)
		: cus(cus_), streams(streams_), n(n_), packed(packed_), patches(patches_), npatches(npatches_), flags(flags_), cut(cut_) {}

	const int lean = lean_policy(flags);
	const bool k2_allowed = lean != 0;
	const bool prefix_allowed = prefix_policy(flags);
	const int variant = pick_variant();
	LevelCut lv[16];
	std::vector<uint8_t> has_patch;
	std::vector<std::vector<uint64_t>> patch_rows;          /* per stream: the rows its patches sit in, sorted */
	std::vector<PatchWindow> windows;
	std::vector<uint8_t> plane_shift;               /* levels 13-15: planes carry values scaled by 2^(16 - level) */
	std::vector<uint8_t> on_tile_kernel;            /* patched stream that stays on the tile kernel: its patches live in windows only */

	int index_patches();
	void count_high_levels();
	uint64_t plane_run(uint64_t elems);
	void to_stagewise(uint32_t id, uint32_t level, uint64_t elems, uint64_t n_emit);
	int cut_lean(size_t i, uint64_t row0, uint64_t rows2, uint32_t T2);
	void cut_patched_fused(size_t i, const AcmDevStream &d);
	int cut_plain_fused(size_t i);
	int cut_prefix(size_t i, const AcmDevStream &d);
	int cut_stream(size_t i);
	int resolve_patches();
	void choose_fused(uint32_t level);
	void choose_tables();
	int run();
};

int Cutter::index_patches()
{
	has_patch.assign(n, 0);
	for (size_t p = 0; p < npatches; p++) {
		if (patches[p].stream >= n) {
			set_err("patch %zu names stream %u of %zu", p, patches[p].stream, n);
			return ACMHIP_ERR_ARG;
		}
		has_patch[patches[p].stream] = 1;
	}
	patch_rows.resize(npatches ? n : 0);
	for (size_t p = 0; p < npatches; p++)
		patch_rows[patches[p].stream].push_back(patches[p].sample >> streams[patches[p].stream].level);
	for (auto &v : patch_rows)
		std::sort(v.begin(), v.end());
	return ACMHIP_OK;
}

/* levels 13 and 14: four rows / two rows are one 128 KB tile of the lean kernel.  Whether a batch is worth its one
 * lead-in tile per workgroup is known only from all its streams: counted here, decided before the streams are cut */
void Cutter::count_high_levels()
{
	for (uint32_t l = ACM_K1_MAX_LEVEL + 1; l <= ACM_K2_MAX_LEVEL; l++) {
		const uint32_t TH = (uint32_t)acmk_tile2_rows(l);
		uint64_t whole = 0;
		for (size_t i = 0; i < n && TH; i++) {
			const acmhip_stream_desc &s = streams[i];
			if (s.level == l && s.row_begin == 0 && !has_patch[i])
				whole += std::min<uint64_t>(s.nrows, s.n_emit >> l) / TH;
		}
		const size_t gridh = (size_t)acmk_tile2_grid(l, cus);
		lv[l].k2_high = k2_allowed && prefix_allowed && TH && gridh && (lean == 1 ? whole > 0 : whole >= 8 * gridh);
	}
}

/* a run of the int32 planes (64-element granules): where it starts */
uint64_t Cutter::plane_run(uint64_t elems)
{
	const uint64_t at = cut.plane_elems;
	cut.plane_elems += (elems + 63) & ~63ull;
	cut.sw_max_elems = std::max(cut.sw_max_elems, elems);
	return at;
}

/* stream `id` (a real one, or a window) joins the stage-wise kernels of its level */
void Cutter::to_stagewise(uint32_t id, uint32_t level, uint64_t elems, uint64_t n_emit)
{
	LevelCut &L = lv[level];
	L.list.push_back(id);
	cut.sw_all.push_back(id);
	L.max_elems = std::max(L.max_elems, elems);
	L.max_emit = std::max(L.max_emit, n_emit);
}

/* rows [row0, row0 + rows2) of stream i as records of the lean tile kernel (T2 rows each), and, where the stream came with a second
 * staged form, once more as records of the build that reads it.  row0 = 0: the stream from its first row (the first record is
 * ACM_TILE_FRESH); row0 > 0 (a multiple of T2; byte-plane streams only): a window - the records start with one for the tile in front
 * of row0, marked ACM_TILE_DISCARD, which builds the carries and stores nothing */
int Cutter::cut_lean(size_t i, uint64_t row0, uint64_t rows2, uint32_t T2)
{
	const acmhip_stream_desc &s = streams[i];
	LevelCut &L = lv[s.level];
	const LeanRows w{ s, row0, s.rows == 1 ? 0u : (uint32_t)(((1ull << 32) + s.rows - 1) / s.rows) };
	if (packed && packed[i].ntiles && packed[i].form > ACMHIP_FORM_BYTEPLANE) {
		set_err("stream %zu: staged form %u", i, packed[i].form);
		return ACMHIP_ERR_ARG;
	}
	const bool pk = packed && packed[i].ntiles && packed[i].form == ACMHIP_FORM_PACKED && acmk_tile2p_rows(s.level) == (int)T2 && row0 == 0;
	/* the matrix-core build may cut the same rows into smaller tiles (its rows in front cost nothing): T2M divides T2 */
	const uint32_t T2M = (uint32_t)acmk_tile2m_rows(s.level);
	const bool mf = packed && packed[i].ntiles && packed[i].form == ACMHIP_FORM_BYTEPLANE && T2M && T2 % T2M == 0;
	if ((pk && packed[i].ntiles < rows2 / T2) || (mf && packed[i].ntiles < (row0 + rows2) / T2M)) {
		set_err("stream %zu: %u tiles in its second staged form, %llu whole tiles to decode", i, packed[i].ntiles,
			(unsigned long long)((row0 + rows2) / (mf ? T2M : T2)));
		return ACMHIP_ERR_ARG;
	}
	if (row0 && (!mf || row0 % T2 || row0 < T2)) {
		set_err("stream %zu: a window on the lean kernels starts on a tile boundary of a stream with a byte-plane form", i);
		return ACMHIP_ERR_ARG;
	}
	/* (a batch of small streams cuts millions of records, on the thread that feeds the device: block and row of a record by
	 * 32-bit division - rows < 2^32 - and room in the vectors made per stream, not per record) */
	const uint64_t first = row0 ? row0 - T2 : 0, ntile = (row0 + rows2 - first) / T2;
	const uint64_t lead_rows = mf ? (uint64_t)T2M * (uint64_t)acmk_tile2m_lead_in(s.level) : 0;      /* (<= T2: two rows more at most) */
	if (row0 && lead_rows > T2) {
		/* the records of a window's lead-in are cut from ONE tile in front of it; a build whose first pass needs more rows than
		 * that in front (level 14: two tiles of two rows) cannot take a window - its streams only ever come here from row 0
		 * (refused loudly instead of decoded wrong, should a caller ever ask) */
		set_err("stream %zu: a window on the lean kernel of level %u needs %llu rows in front, a tile has %u", i, s.level,
			(unsigned long long)lead_rows, T2);
		return ACMHIP_ERR_ARG;
	}
	if (pk || mf)
		cut.form_rows[i] = rows2;
	std::vector<AcmTile2> &plain = pk ? L.tiles2p_plain : mf ? L.tiles2m_plain : L.tiles2;
	const uint32_t pk_slots = pk ? (uint32_t)acmk_tile2p_slots(s.level) : 0;
	const bool twin = !(mf && (flags & ACMHIP_PLAN_FORM_ONLY));
	if (twin)
		room(plain, ntile);
	if (pk)
		room(L.tiles2p, ntile);
	if (mf)
		room(L.tiles2m, ntile * (T2 / T2M));
	const uint32_t srows = s.rows;
	for (uint64_t r = first; r < row0 + rows2; r += T2) {
		const bool lead_in = r < row0;
		const uint32_t rh = (uint32_t)(r >= 2 ? r - 2 : 0);         /* the row the row-value fetch counts from */
		if (twin)
			plain.push_back(AcmTile2{ s.idx_off + (r << s.level), w.pcm_of(r), (uint32_t)(s.hdr_off + rh / srows), rh % srows, w.magic,
						  w.flags_of(r, lead_in) });
		if (pk)
			L.tiles2p.push_back(AcmTile2{ packed[i].chunk_off + r / T2 * (uint64_t)pk_slots, s.pcm_off + (r << s.level),
						      (uint32_t)(s.hdr_off + (uint32_t)r / srows), (uint32_t)r % srows, w.magic,
						      r == 0 ? ACM_TILE_FRESH : 0u });
		if (mf)
			cut_chunks(L.tiles2m, w, packed[i].chunk_off, r, lead_in, T2, T2M, lead_rows);
	}
	return ACMHIP_OK;
}

/* a patched stream of the fused kernel's levels: its clean tiles stay there (halo flavour, outside any carry run), every tile that can
 * see a patched sample - in its own rows or its two halo rows - becomes a window for the stage-wise kernels */
void Cutter::cut_patched_fused(size_t i, const AcmDevStream &d)
{
	const acmhip_stream_desc &s = streams[i];
	on_tile_kernel[i] = 1;
	const uint32_t T = (uint32_t)acmk_fused_tile_rows(s.level, variant) - 2;
	const uint64_t cols = 1ull << s.level;
	const uint64_t emit_rows = (s.n_emit + cols - 1) >> s.level;
	const std::vector<uint64_t> &pr = patch_rows[i];
	for (uint64_t r = 0; r < emit_rows; r += T) {
		const uint64_t row0 = s.row_begin + r;
		const uint64_t lo = row0 >= 2 ? row0 - 2 : 0, hi = std::min<uint64_t>(row0 + T, s.nrows);
		auto it = std::lower_bound(pr.begin(), pr.end(), lo);
		if (it == pr.end() || *it >= hi) {
			lv[s.level].tiles_extra.push_back(AcmTile{ (uint32_t)i, (int32_t)row0, 0u, 0u });
			continue;
		}
		AcmDevStream w = d;
		w.pcm_off = s.pcm_off + (r << s.level);
		w.n_emit = std::min<uint64_t>((uint64_t)T << s.level, s.n_emit - (r << s.level));
		w.row_begin = (uint32_t)row0;
		w.halo_row = (uint32_t)lo;
		w.nrows = (uint32_t)hi;
		const uint64_t elems = (hi - lo) << s.level;
		w.scratch_off = plane_run(elems);
		windows.push_back(PatchWindow{ (uint32_t)i, lo, hi, w.scratch_off });
		const uint32_t id = (uint32_t)cut.streams.size();
		cut.streams.push_back(w);
		to_stagewise(id, s.level, elems, w.n_emit);
	}
}

/* a stream of the fused kernel's levels without patches: cut every way its level may launch it - halo tiles throughout; whole tiles on
 * the lean kernels and the rest as halo tiles; carry tiles - and choose_fused() picks once the level's tile counts are known */
int Cutter::cut_plain_fused(size_t i)
{
	const acmhip_stream_desc &s = streams[i];
	LevelCut &L = lv[s.level];
	const uint32_t T = (uint32_t)acmk_fused_tile_rows(s.level, variant) - 2;
	const uint64_t cols = 1ull << s.level;
	const uint64_t emit_rows = (s.n_emit + cols - 1) >> s.level;
	for (uint64_t r = 0; r < emit_rows; r += T)
		L.tiles.push_back(AcmTile{ (uint32_t)i, (int32_t)(s.row_begin + r), 0u, 0u });
	/* the lean kernel takes the whole tiles of a stream that is decoded from its row 0; the ragged tail
	 * (and every other kind of stream) stays with the general kernel, as halo tiles */
	const uint32_t T2 = (uint32_t)acmk_tile2_rows(s.level);
	uint64_t rows2 = 0;
	if (k2_allowed && T2 && s.row_begin == 0) {
		const uint64_t full_rows = std::min<uint64_t>(s.nrows, s.n_emit >> s.level);
		rows2 = full_rows / T2 * T2;
		const int cr = cut_lean(i, 0, rows2, T2);
		if (cr != ACMHIP_OK)
			return cr;
	} else if (k2_allowed && T2 && s.row_begin >= T2 && s.row_begin % T2 == 0 && packed && packed[i].ntiles &&
		   packed[i].form == ACMHIP_FORM_BYTEPLANE && acmk_tile2m_rows(s.level) > 0 && T2 % (uint32_t)acmk_tile2m_rows(s.level) == 0) {
		/* a window that starts on a tile boundary of a stream with a byte-plane form (a block range of a device-parsed batch):
		 * its whole tiles go to the lean kernels too, behind a lead-in record for the tile in front of it */
		const uint64_t full_rows = std::min<uint64_t>(s.nrows - s.row_begin, s.n_emit >> s.level);
		rows2 = full_rows / T2 * T2;
		if (rows2) {
			const int cr = cut_lean(i, s.row_begin, rows2, T2);
			if (cr != ACMHIP_OK)
				return cr;
		}
	}
	for (uint64_t r = rows2; r < emit_rows; r += T)
		L.tiles_rest.push_back(AcmTile{ (uint32_t)i, (int32_t)(s.row_begin + r), 0u, 0u });
	if (acmk_fused_has_carry(s.level, variant))
		cut_carry(L.tiles_carry, (uint32_t)i, s.row_begin, emit_rows, T + 2);   /* carry mode: T + 2 payload rows per tile */
	return ACMHIP_OK;
}

/* levels 13-15: level - 12 stages by the stage-wise kernels into a plane (scaled, see acmk_launch_unpack), then the plane is a level-12
 * stream of 2^(level-12) times as many rows for the tile kernel: stage k of level L has the stride of stage k - j of level L - j, and
 * the "+1" belongs to stage 0 alone (decode.c:555-571) */
int Cutter::cut_prefix(size_t i, const AcmDevStream &d)
{
	const acmhip_stream_desc &s = streams[i];
	LevelCut &L = lv[s.level];
	uint32_t sid = (uint32_t)i;             /* the stream the prefix + plane pair works on: this one, or the rest of it */
	AcmDevStream src = d;
	if (L.k2_high && s.row_begin == 0 && !has_patch[i]) {
		/* the whole tiles go to the lean tile kernel; whatever is left - the ragged tail - is a window of the
		 * stream (a pseudo stream behind the n real ones) for the prefix + plane pair */
		const uint32_t T2 = (uint32_t)acmk_tile2_rows(s.level);
		const uint64_t rows2 = std::min<uint64_t>(s.nrows, s.n_emit >> s.level) / T2 * T2;
		const int cr = cut_lean(i, 0, rows2, T2);
		if (cr != ACMHIP_OK)
			return cr;
		if (rows2 > 0) {
			src.pcm_off = s.pcm_off + (rows2 << s.level);
			src.n_emit = s.n_emit - (rows2 << s.level);
			src.row_begin = (uint32_t)rows2;
			src.halo_row = (uint32_t)rows2 - 2;
			if (src.n_emit) {
				sid = (uint32_t)cut.streams.size();
				cut.streams.push_back(src);
			}
		}
	}
	if (src.n_emit) {
		const uint32_t j = s.level - 12;
		const uint64_t elems = (uint64_t)(src.nrows - src.halo_row) << s.level;
		AcmDevStream w{};
		w.idx_off = plane_run(elems);                   /* int32 units into the plane */
		cut.streams[sid].scratch_off = w.idx_off;
		if (sid < n)
			plane_shift[sid] = (uint8_t)(16 - s.level);
		w.pcm_off = src.pcm_off;
		w.n_emit = src.n_emit;
		w.level = 12;
		w.rows = 1;
		w.nrows = (src.nrows - src.halo_row) << j;
		w.row_begin = (src.row_begin - src.halo_row) << j;
		w.halo_row = w.row_begin >= 2 ? w.row_begin - 2 : 0;
		const uint32_t id = (uint32_t)cut.streams.size();
		cut.streams.push_back(w);
		const uint32_t T12 = (uint32_t)acmk_plane_tile_rows() - 2;
		const uint64_t emit_rows = (src.n_emit + 4095) >> 12;
		for (uint64_t r = 0; r < emit_rows; r += T12)
			L.prefix_tiles.push_back(AcmTile{ id, (int32_t)(w.row_begin + r), 0u, 0u });
		cut_carry(L.prefix_tiles_carry, id, w.row_begin, emit_rows, T12 + 2);
		L.prefix_list.push_back(sid);
		L.max_elems = std::max(L.max_elems, elems);
	}
	return ACMHIP_OK;
}

/* stream i: checked, its AcmDevStream written, its rows handed to the kernel family that decodes them */
int Cutter::cut_stream(size_t i)
{
	const acmhip_stream_desc &s = streams[i];
	if (!valid_desc(s)) {
		set_err("stream %zu: invalid descriptor (level %u rows %u nrows %u row_begin %u n_emit %llu idx_off %llu pcm_off %llu)",
			i, s.level, s.rows, s.nrows, s.row_begin, (unsigned long long)s.n_emit,
			(unsigned long long)s.idx_off, (unsigned long long)s.pcm_off);
		return ACMHIP_ERR_ARG;
	}
	/* the lean records name a block header and (byte-plane form) a pair-table entry in 32 bits: a stream whose last header, or whose
	 * last pair entry with the table's read slack behind it, does not fit is refused here, whatever kernel family it would go to -
	 * never wrapped */
	const uint64_t blocks = ((uint64_t)s.nrows + s.rows - 1) / s.rows;
	if (s.hdr_off > ACM_TABLE_INDEX_END - blocks) {
		set_err("stream %zu: hdr_off %llu + %llu blocks is past header %llu, the last a launch can name", i, (unsigned long long)s.hdr_off,
			(unsigned long long)blocks, (unsigned long long)(ACM_TABLE_INDEX_END - 1));
		return ACMHIP_ERR_ARG;
	}
	if (packed && packed[i].ntiles && packed[i].form == ACMHIP_FORM_BYTEPLANE) {
		const uint64_t entries = (uint64_t)packed[i].ntiles * (uint64_t)std::max(acmk_tile2m_rows(s.level), 0) / 2 + 1 + ACM_PAIR_READ_SLACK;
		if (entries > ACM_TABLE_INDEX_END || packed[i].chunk_off > ACM_TABLE_INDEX_END - entries) {
			set_err("stream %zu: chunk_off %llu + %llu pair-table entries (%u of them read slack) is past entry %llu, the last a launch can name",
				i, (unsigned long long)packed[i].chunk_off, (unsigned long long)entries, (unsigned)ACM_PAIR_READ_SLACK,
				(unsigned long long)(ACM_TABLE_INDEX_END - 1));
			return ACMHIP_ERR_ARG;
		}
	}
	const AcmDevStream d = dev_stream_of(s);        /* by value: cut.streams grows while windows are cut */
	cut.streams[i] = d;
	cut.stats.samples += s.n_emit;
	if (s.n_emit == 0)
		return ACMHIP_OK;

	int rc = ACMHIP_OK;
	const bool stagewise = (flags & ACMHIP_PLAN_STAGEWISE) != 0;
	if (!stagewise && fused_ok(s, variant)) {
		if (has_patch[i])
			cut_patched_fused(i, d);
		else
			rc = cut_plain_fused(i);
	} else if (!stagewise && s.level <= ACM_SMALL_MAX_LEVEL && !has_patch[i]) {
		lv[s.level].small_list.push_back((uint32_t)i);
		lv[s.level].max_emit = std::max(lv[s.level].max_emit, (uint64_t)s.n_emit);
	} else if (prefix_allowed && s.level > ACM_K1_MAX_LEVEL) {
		rc = cut_prefix(i, d);
	} else {
		const uint64_t elems = (uint64_t)(s.nrows - d.halo_row) << s.level;
		cut.streams[i].scratch_off = plane_run(elems);
		to_stagewise((uint32_t)i, s.level, elems, s.n_emit);
		cut.stats.stagewise_streams++;
		return ACMHIP_OK;
	}
	cut.stats.fused_streams++;
	return rc;
}

/* H1 patches -> plane coordinates */
int Cutter::resolve_patches()
{
	std::vector<AcmDevPatch> &dp = cut.patches;
	std::vector<std::vector<size_t>> win_of(windows.empty() ? 0 : n);
	for (size_t w = 0; w < windows.size(); w++)
		win_of[windows[w].stream].push_back(w);
	for (size_t p = 0; p < npatches; p++) {
		const AcmDevStream &d = cut.streams[patches[p].stream];
		if (on_tile_kernel[patches[p].stream]) {
			/* a tile-kernel stream: the patch lands in every window that can see it (its own tile, and the next one
			 * when it sits in that tile's two halo rows); a patch no window sees (behind the last emitted tile, or
			 * outside a windowed decode) changes nothing that is emitted and has no place in the plane: the stream
			 * owns no plane run of its own (scratch_off 0 is somebody else's) */
			const uint64_t row = patches[p].sample >> d.level;
			if (win_of.empty())
				continue;
			for (size_t w : win_of[patches[p].stream]) {
				const PatchWindow &pw = windows[w];
				if (row >= pw.lo_row && row < pw.hi_row)
					dp.push_back(AcmDevPatch{ pw.scratch_off + (patches[p].sample - (pw.lo_row << d.level)), patches[p].value, 0 });
			}
			continue;
		}
		const uint64_t first = (uint64_t)d.halo_row << d.level;
		const uint64_t end = (uint64_t)d.nrows << d.level;
		if (d.n_emit == 0 || patches[p].sample < first || patches[p].sample >= end)
			continue;
		dp.push_back(AcmDevPatch{ d.scratch_off + (patches[p].sample - first),
					  (int32_t)((uint32_t)patches[p].value << plane_shift[patches[p].stream]), 0 });
	}
	for (const AcmDevPatch &q : dp)
		if (q.dst >= cut.plane_elems) {
			set_err("internal: H1 patch lands at %llu of a %llu-element plane", (unsigned long long)q.dst,
				(unsigned long long)cut.plane_elems);
			return ACMHIP_ERR_ARG;
		}
	return ACMHIP_OK;
}

/* the fused group of a level: lean kernels or not, and which flavour of the fused kernel's table goes with that */
void Cutter::choose_fused(uint32_t level)
{
	LevelCut &L = lv[level];
	acmhip_plan_stats &st = cut.stats;
	AcmCutGroup g;
	g.level = level;
	if (!L.tiles_extra.empty()) {
		st.tiles += L.tiles_extra.size();
		st.launches += 1;
		if (L.tiles.empty())
			st.launches -= 1;               /* the launch counted below does not happen */
		g.tiles_extra = std::move(L.tiles_extra);
	}
	const size_t grid = (size_t)acmk_fused_grid(level, variant, cus);
	/* the lean kernel replays one tile per workgroup as a lead-in: worth it from a few tiles per workgroup on */
	const size_t grid2 = (size_t)acmk_tile2_grid(level, cus);
	const size_t n2 = L.tiles2.size() + L.tiles2p.size() + L.tiles2m.size();
	/* streams that came with a packed form always take the lean kernel: their caller may have staged nothing else for
	 * these rows (acm_batch_decode with ACM_BATCH_STAGE_PACKED uploads the int16 form of the ragged tails only) */
	const bool k2 = grid2 && (level > ACM_K1_MAX_LEVEL ? n2 > 0         /* levels 13, 14: decided before the cut */
				  : lean == 1 ? n2 > 0 : (n2 >= 8 * grid2 || !L.tiles2p.empty() || !L.tiles2m.empty()));
	g.carry = !k2 && !L.tiles_carry.empty() && carry_wanted(L.tiles_carry.size(), grid, (size_t)acmk_fused_tile_rows(level, variant), flags);
	g.tiles = std::move(k2 ? L.tiles_rest : g.carry ? L.tiles_carry : L.tiles);
	if (k2) {
		cut.need_sink = true;
		st.tiles += L.tiles2.size() + L.tiles2p.size() + L.tiles2m.size();
		st.launches += (L.tiles2.empty() ? 0 : 1) + (L.tiles2p.empty() ? 0 : 1) + (L.tiles2m.empty() ? 0 : 1);
		st.packed_tiles += L.tiles2p.size();
		st.mform_tiles += L.tiles2m.size();
		if (g.tiles.empty())
			st.launches -= 1;
		g.tiles2 = std::move(L.tiles2);
		g.tiles2p = std::move(L.tiles2p);
		g.tiles2p_plain = std::move(L.tiles2p_plain);
		g.tiles2m = std::move(L.tiles2m);
		g.tiles2m_plain = std::move(L.tiles2m_plain);
	}
	st.tiles += g.tiles.size();
	st.launches += 1;
	cut.fused.push_back(std::move(g));
}

/* per level: the groups a launch walks, with the tables they use, and what that comes to in tiles and launches */
void Cutter::choose_tables()
{
	acmhip_plan_stats &st = cut.stats;
	for (uint32_t level = 0; level < 16; level++) {
		LevelCut &L = lv[level];
		if (!L.tiles.empty() || !L.tiles_extra.empty() || !L.tiles2.empty() || !L.tiles2p.empty() || !L.tiles2m.empty())
			choose_fused(level);
		if (!L.small_list.empty()) {
			AcmCutGroup g;
			g.level = level;
			g.max_emit = L.max_emit;
			g.list = std::move(L.small_list);
			cut.small.push_back(std::move(g));
			st.launches += 1;
		}
		if (!L.prefix_list.empty()) {
			AcmCutGroup g;
			g.level = level;
			g.prefix_stages = level - 12;
			for (uint32_t id : L.prefix_list)
				g.prefix_patched = g.prefix_patched || (id < n && has_patch[id]);
			g.max_elems = L.max_elems;
			g.list = std::move(L.prefix_list);
			g.carry = carry_wanted(L.prefix_tiles_carry.size(), (size_t)acmk_plane_grid(cus), (size_t)acmk_plane_tile_rows(), flags);
			g.tiles = std::move(g.carry ? L.prefix_tiles_carry : L.prefix_tiles);
			st.tiles += g.tiles.size();
			st.launches += g.prefix_patched ? 2 + g.prefix_stages : 2;           /* prefix sweep (or unpack + stages), tile kernel */
			cut.prefix.push_back(std::move(g));
		}
		if (!L.list.empty()) {
			AcmCutGroup g;
			g.level = level;
			g.max_elems = L.max_elems;
			g.max_emit = L.max_emit;
			g.list = std::move(L.list);
			cut.stagewise.push_back(std::move(g));
			st.launches += level + 1;          /* stages + emit */
		}
	}
	if (cut.plane_elems > 0) {
		st.launches += cut.sw_all.empty() ? 0 : 1;      /* unpack */
		st.launches += cut.patches.empty() ? 0 : 1;
	}
}

int Cutter::run()
{
	int rc = index_patches();
	if (rc != ACMHIP_OK)
		return rc;
	cut.streams.resize(n);
	cut.form_rows.assign(n, 0);
	cut.variant = variant;
	cut.form_only = (flags & ACMHIP_PLAN_FORM_ONLY) != 0;
	plane_shift.assign(n, 0);
	on_tile_kernel.assign(n, 0);
	count_high_levels();
	for (size_t i = 0; i < n && rc == ACMHIP_OK; i++)
		rc = cut_stream(i);
	if (rc == ACMHIP_OK)
		rc = resolve_patches();
	if (rc == ACMHIP_OK)
		choose_tables();
	return rc;
}

} // namespace

int acm_plan_cut(int cus, const acmhip_stream_desc *streams, size_t n, const acmhip_packed_stream *packed,
		 const acmhip_patch *patches, size_t npatches, unsigned flags, AcmPlanCut *out)
{
	if (!out || (n && !streams) || (npatches && !patches) || n > 0xFFFFFFFFull)
		return ACMHIP_ERR_ARG;
	*out = AcmPlanCut{};
	Cutter c(cus, streams, n, packed, patches, npatches, flags, *out);
	return c.run();
}

extern "C" int acmk_plan_cut_visit(int cus, const acmhip_stream_desc *streams, size_t n, const acmhip_packed_stream *packed,
				   const acmhip_patch *patches, size_t npatches, unsigned flags, acmk_cut_visit visit, void *ctx)
{
	AcmPlanCut cut;
	const int rc = acm_plan_cut(cus, streams, n, packed, patches, npatches, flags, &cut);
	if (rc != ACMHIP_OK || !visit)
		return rc;
	auto show = [&](const char *name, uint32_t level, const auto &v) {
		if (!v.empty())
			visit(ctx, name, level, v.data(), sizeof(v[0]), v.size());
	};
	show("streams", 0, cut.streams);
	const std::vector<AcmCutGroup> *kinds[4] = { &cut.fused, &cut.small, &cut.prefix, &cut.stagewise };
	static const char *const list_name[4] = { "", "small_list", "prefix_list", "sw_list" };
	std::vector<uint64_t> words(sizeof(cut.stats) / 8);
	memcpy(words.data(), &cut.stats, sizeof(cut.stats));
	const uint64_t head[4] = { cut.plane_elems, cut.sw_max_elems, cut.need_sink, cut.fused.size() + cut.small.size() + cut.prefix.size() + cut.stagewise.size() };
	words.insert(words.end(), head, head + 4);
	for (uint64_t k = 0; k < 4; k++)
		for (const AcmCutGroup &g : *kinds[k]) {
			show(k == 2 ? "prefix_tiles" : "tiles", g.level, g.tiles);
			show("tiles_extra", g.level, g.tiles_extra);
			show("tiles2", g.level, g.tiles2);
			show("tiles2p", g.level, g.tiles2p);
			show("tiles2p_plain", g.level, g.tiles2p_plain);
			show("tiles2m", g.level, g.tiles2m);
			show("tiles2m_plain", g.level, g.tiles2m_plain);
			show(list_name[k], g.level, g.list);
			const uint64_t rec[7] = { k, g.level, g.carry, g.max_elems, g.max_emit, g.prefix_patched, g.prefix_stages };
			words.insert(words.end(), rec, rec + 7);
		}
	show("sw_all", 0, cut.sw_all);
	show("patches", 0, cut.patches);
	show("form_rows", 0, cut.form_rows);
	show("stats", 0, words);
	return rc;
}
