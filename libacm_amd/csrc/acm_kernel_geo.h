/*
 * acm_kernel_geo.h - the launch geometry of every kernel build, written once: how big a tile is, how many threads work on it, how many
 * workgroups a CU holds, how deep a first pass is.  Constant expressions only - no HIP header, nothing __device__ - so that two readers
 * see the same text:
 *   acm_kernels.hip      instantiates its kernels from the build traits below (entry_k2<Tile2Build<9>, 3, 3, 3>());
 *   acm_kernel_geo.cpp   answers the planner's and the stagers' acmk_* queries from the same tables, without a device and without a kernel.
 * What is NOT here: the stage groupings (Gs...) of a build - they change what a kernel does, not what the host has to cut - and every kernel.
 *
 * A build made with -D flags that change a number below (profiles/build_variant.sh) must compile BOTH readers with them: digest() is
 * exported by each and acmhip_device_open refuses a library whose two halves disagree.
 */
#ifndef ACM_KERNEL_GEO_H
#define ACM_KERNEL_GEO_H

#include <stdint.h>

#include <initializer_list>

#include "acm_device.h"

/* variants 1.. of the fused kernel are tuning aids (geometry sweeps: -DACM_TUNING; timing-only ablations: -DACM_ABLATION, which implies it) */
#if defined(ACM_ABLATION) && !defined(ACM_TUNING)
#define ACM_TUNING 1
#endif

namespace acm_geo {

/* tile configuration: level, threads per workgroup, tile elements held in LDS */
template <int L_, int NT_, int NELEM_>
struct TileCfg {
	static constexpr int L = L_;
	static constexpr int NT = NT_;
	static constexpr int NELEM = NELEM_;
	static constexpr int COLS = 1 << L_;
	static constexpr int TR = NELEM_ / COLS;          // tile rows incl. the 2 halo rows
	static constexpr int NJ_LAST = NELEM_ / NT_;      // samples per thread in the last pass
	static constexpr int PS = NJ_LAST >= 64 ? 6 : 5;  // LDS pad: one dword per 2^PS elements (= one last-pass walk)
	static_assert(NJ_LAST == 64 || NJ_LAST == 32 || NJ_LAST == 128, "walk length of the last pass");
	static_assert(TR >= 1, "whole rows");
	static constexpr bool ROW_PAIRS = TR >= 2 && (TR % 2) == 0;     /* what the first passes fed from HBM work on (the halo flavour of acm_fused_tile needs four rows: two of them are halo) */
};

/* one row of the tables below: threads, tile elements, and `w` - the workgroups a CU holds (acm_tile2 and its kin), or the W of
 * acm_fused_tile (256-thread units of a workgroup: W * 256 / nt workgroups per CU).  nt == 0: the level has no such build */
struct Tile { int nt, nelem, w; };
/* what the host needs of a build */
struct Launch { int threads, tile_rows, wg_per_cu; };
constexpr Launch launch_of(const Tile t, const int level) { return Launch{ t.nt, t.nt ? t.nelem >> level : 0, t.w }; }

// ---------------------------------------------------------------------------
// acm_fused_tile
// ---------------------------------------------------------------------------
/*
 * Kernel variants (ACM_K1_VARIANT=n picks one; tuning aid, see profiles/sweep_variants.py):
 *   0  default: per level the fastest measured geometry
 *   1  256 threads, 16K-element tiles, 2-byte first-pass loads (64 samples per thread per pass)
 *   2  512 threads (32 samples per thread per pass, 16 waves per CU)
 *   3  256 threads on half-size tiles (4 workgroups per CU)
 *   4  as 1 with 4-byte first-pass loads (two adjacent columns per lane)
 *   5  as 1 with fewer, deeper LDS passes
 *   6, 7  alternative stage groupings;  8  128-thread workgroups (128 samples per thread per pass)
 * (carry: the carry-mode build of the same geometry exists too - no halo rows; see ACM_TILE_*)
 */
struct FusedTile { Tile t; bool carry = false; };
#ifdef ACM_ABLATION
constexpr int NVARIANTS = 20;
#elif defined(ACM_TUNING)
constexpr int NVARIANTS = 10;
#else
constexpr int NVARIANTS = 1;
#endif
constexpr FusedTile FUSED[NVARIANTS][ACM_K1_MAX_LEVEL - ACM_K1_MIN_LEVEL + 1] = {
	/* variant 0 (default): per level the fastest measured geometry (profiles/sweep_variants.py) */
	{ { { 128, 8192, 2 }, true }, { { 256, 16384, 2 }, true }, { { 256, 16384, 2 }, true }, { { 256, 16384, 2 }, true }, { { 256, 16384, 2 }, true },
	  { { 256, 16384, 2 }, true }, { { 512, 32768, 2 }, true }, { { 512, 32768, 2 }, true } },
#ifdef ACM_TUNING
	/* variant 1: 64 KB tiles shared by 8 waves (4 waves per SIMD, 32 elements per thread) */
	{ { { 128, 8192, 2 } }, { { 512, 16384, 4 } }, { { 512, 16384, 4 } }, { { 512, 16384, 4 } }, { { 512, 16384, 4 } }, { { 512, 32768, 2 } }, { { 512, 32768, 2 } } },
	/* variant 2: 128 KB tiles (one workgroup of 8 waves per CU): half the halo share of the 64 KB tiles */
	{ { { 128, 8192, 2 } }, { { 512, 32768, 2 } }, { { 512, 32768, 2 } }, { { 512, 32768, 2 } }, { { 512, 32768, 2 } }, { { 512, 32768, 2 } }, { { 512, 32768, 2 } } },
	/* variant 3 */
	{ { { 256, 8192, 4 } }, { { 256, 8192, 4 } }, { { 256, 8192, 4 } }, { { 256, 8192, 4 } }, { { 256, 8192, 4 } }, { { 512, 16384, 4 } }, { { 512, 32768, 2 } } },
	/* variants 4, 5 */
	{ { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 32768, 1 } } },
	{ { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 32768, 1 } } },
	/* variants 6, 7: alternative stage groupings (tuning) */
	{ { { 256, 8192, 4 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 512, 32768, 2 } } },
	{ { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 512, 32768, 2 } } },
	/* variant 8: 128-thread workgroups, 128 samples per thread per pass (half the warm-up share) */
	{ { { 128, 8192, 2 } }, { { 128, 16384, 1 } }, { { 128, 16384, 1 } }, { { 128, 16384, 1 } }, { { 128, 16384, 1 } }, { { 128, 16384, 1 } }, { { 256, 32768, 1 } } },
	/* variant 9: 32 KB tiles, four workgroups per CU (4 waves per SIMD), carry mode */
	{ { { 128, 8192, 2 }, true }, { { 256, 8192, 4 }, true }, { { 256, 8192, 4 }, true }, { { 256, 8192, 4 }, true }, { { 256, 8192, 4 }, true },
	  { { 256, 16384, 2 }, true }, { { 512, 32768, 2 }, true }, { { 512, 32768, 2 }, true } },
#endif
#ifdef ACM_ABLATION
	/* variant 10 (timing only): the default geometry without the barriers inside the LDS passes; 11-19: the geometry of variant 5 with parts removed */
	{ { { 128, 8192, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 512, 32768, 2 } } },
#define ACM_GEO_ABL_ROW { { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 16384, 2 } }, { { 256, 32768, 1 } } }
	ACM_GEO_ABL_ROW, ACM_GEO_ABL_ROW, ACM_GEO_ABL_ROW, ACM_GEO_ABL_ROW, ACM_GEO_ABL_ROW, ACM_GEO_ABL_ROW, ACM_GEO_ABL_ROW, ACM_GEO_ABL_ROW, ACM_GEO_ABL_ROW,
#undef ACM_GEO_ABL_ROW
#endif
};
constexpr Launch fused_launch(const FusedTile f, const int level) { return Launch{ f.t.nt, f.t.nt ? f.t.nelem >> level : 0, f.t.nt ? f.t.w * 256 / f.t.nt : 0 }; }
template <int V, int L_>
struct FusedBuild {
	static constexpr FusedTile F = FUSED[V][L_ - ACM_K1_MIN_LEVEL];
	static_assert(F.t.nt != 0, "this variant has no build of the level");
	using C = TileCfg<L_, F.t.nt, F.t.nelem>;
	static constexpr int W = F.t.w;
	static constexpr bool CARRY = F.carry;
};

/* levels 13-15: the stage-wise kernels apply the first level-12 stages into an int32 plane, this level-12 build of the tile
 * kernel (one 128 KB tile per CU - two 64 KB tiles spill with the 64 prefetch registers of a plane; halo or carry flavour like
 * every other group) reads the plane and does the other twelve */
constexpr FusedTile PLANE = { { 512, 32768, 2 }, true };
struct PlaneBuild {
	using C = TileCfg<12, PLANE.t.nt, PLANE.t.nelem>;
	static constexpr int W = PLANE.t.w;
};

// ---------------------------------------------------------------------------
// acm_tile2
// ---------------------------------------------------------------------------
/* per level the fastest measured geometry and stage grouping (profiles/r2_sweep_levels.txt): 32 KB tiles at four workgroups
 * per CU up to level 10, 64 KB tiles of 512 threads (two workgroups, still four waves per SIMD) above; passes of at most
 * three stages, because with 32-element walks the warm-up of a four-stage pass costs as much as a pass */
/* per level the fastest measured geometry and stage grouping with the phase priorities on (profiles/r2_sweep_levels.txt;
 * alternatives built and timed on one box, all CRC-verified: level 7 (2,2,3) and (2,3,2) -2 %; level 8 (2,3,3), (3,2,3)
 * equal; level 9 as 64 KB tiles of 512 threads -0.4 %; level 10 (2,3,3,2) -1.5 %, (2,2,3,3) -2.5 %, 64 KB tiles -1.5 %;
 * level 11 as 64 KB tiles of 512 threads, two per CU, (2,3,3,3): -2.7 %, which had been the best without priorities) */
constexpr Tile TILE2[ACM_K2_MAX_LEVEL - ACM_K2_MIN_LEVEL + 1] = {
	{ 256, 8192, 4 }, { 256, 8192, 4 }, { 256, 8192, 4 }, { 256, 8192, 4 }, { 256, 8192, 4 }, { 256, 8192, 4 },
	{ 512, 16384, 2 },      /* two 64 KB tiles per CU (127 registers): +19 % over one 128 KB tile, whose waves are all in the same phase */
	/* level 13: four rows are 128 KB - one workgroup of sixteen waves per CU (still four per SIMD), no plane, no prefix sweep:
	 * 4 B of HBM traffic per sample instead of the 12 B of the prefix + plane pair.  A two-stage first pass makes the
	 * whole tile ONE segment (1024 threads x two adjacent columns = the 2048 residues of stride 2048): two warm-up rows per
	 * four rows instead of per two, 24 instead of 32 prefetch registers: +8 % over (3,2,3,3,2) (2.94 against 3.18 ms for
	 * 2.1 Gsamples; at levels 10 and 11 the same trade loses 3 %: an LDS-pass stage costs more than a first-pass stage) */
	{ 1024, 32768, 1 },
	/* level 14: one row pair is the 128 KB tile (the first pass's body is two rows: the least a tile can be), 155 KB of LDS
	 * with the carries of the first LDS pass (two bodies of stride 256 = 4096 elements) */
	{ 1024, 32768, 1 },
};
/* C: the tile; WPC: workgroups per CU; W: acm_tile2's count of 256-thread units per CU */
template <int L_, int NT_, int NELEM_, int WPC_>
struct TileBuildOf {
	using C = TileCfg<L_, NT_, NELEM_>;
	static constexpr int WPC = WPC_, W = WPC_ * NT_ / 256;
};
template <int L_>
struct Tile2Build : TileBuildOf<L_, TILE2[L_ - ACM_K2_MIN_LEVEL].nt, TILE2[L_ - ACM_K2_MIN_LEVEL].nelem, TILE2[L_ - ACM_K2_MIN_LEVEL].w> {};

// ---------------------------------------------------------------------------
// acm_chunk: what ONE wavefront works on
// ---------------------------------------------------------------------------
#ifndef ACM_K3_DPP_HISTORY
#define ACM_K3_DPP_HISTORY 1
#endif
template <int L_>
struct ChunkGeo {
	/* what ONE wavefront holds in LDS: 2048 elements (32 per lane in the last pass), or one row where a row is longer (levels 12 and 13:
	 * 4096 / 8192 elements, eight / four wavefronts per workgroup with twice / four times the registers each) */
	static constexpr int NELEM = (1 << L_) > 2048 ? (1 << L_) : 2048;
	using C = TileCfg<L_, 64, NELEM>;
	static constexpr int NW = 32768 / NELEM;                /* wavefronts per workgroup = per CU */
	static constexpr int L = L_, COLS = C::COLS, TR = C::TR, PS = C::PS;
	static constexpr int G = 6, QN = 1 << G, SIGMA = COLS / QN;            /* QN columns of a residue class per row, SIGMA classes */
	static_assert(SIGMA >= 2 && TR >= 1, "sixteen instances per matrix instruction: sixteen classes of one row, or all the classes of 2 / 4 / 8 rows");
	static constexpr int RR = SIGMA >= 16 ? 1 : 16 / SIGMA; /* row walkers among the sixteen instances */
	static constexpr int NG = SIGMA >= 16 ? SIGMA / 16 : 1; /* groups of sixteen classes per row */
	static constexpr int NSW = TR / RR;                     /* rows a walker walks */
	static constexpr int NX = NSW + 2;                      /* rows a lane loads per group: its walk and the two rows in front of it */
	static constexpr int NSET = NSW * NG;                   /* matrix "sets" (sixteen instances x 64 outputs) per chunk: 2048 / 1024 */
	static constexpr int NE = (((TR & 1) + (RR - 1) * NSW + NX - 1) >> 1) + 1;      /* pair-table entries a chunk may read, from the pair in front of it on
										 * (a chunk of one row may start on the second row of a pair) */
	static constexpr int NM = QN / 16;                      /* output tiles per row */
	static_assert(NSW * RR == TR && NSET * 1024 == NELEM, "a chunk is whole sets");
	/* KEEP (one walker only: the rows in front of a lane's walk are rows the SAME lane loaded for the chunk in front): only the walk's own
	 * rows are asked for, the two rows in front stay in their registers (shift_history) - a third (level 11) or half of the requests */
	static constexpr bool HISTORY_IN_REGISTERS = RR == 1;
	/* two walkers of two rows each (level 9): the rows in front of walker 1 are walker 0's own rows of the same chunk, the rows in front of
	 * walker 0 are walker 1's own rows of the chunk before - both sit eight lanes away in the same row of sixteen, one v_mov_b32_dpp per
	 * register instead of a second request for bytes the partner lane has just loaded (half the load instructions of a chunk) */
	/* (round 6: the same with four walkers of two rows each, level 8 - walker w's rows in front are walker w - 1's own, SIGMA lanes down
	 * the row of sixteen; walker 0's are the last walker's of the chunk before, 16 - SIGMA lanes up) */
	static constexpr bool HISTORY_BY_DPP = ACM_K3_DPP_HISTORY && RR >= 2 && NSW == 2 && RR * SIGMA == 16 && SIGMA >= 4;
	static constexpr bool KEEPS_ROWS = HISTORY_IN_REGISTERS || HISTORY_BY_DPP;
	static constexpr Tile TILE = { 64 * NW, NELEM, 1 };     /* a "tile" is one wavefront's chunk; the workgroup is the CU: its wavefronts share the coefficient tables */
};

/* tiles of a build the planner puts in front of a window into a stream (ACM_TILE_DISCARD records): one - every pass reaches back less
 * than a tile - except where a first pass keeps the two rows in front of a walk of `walk_rows` rows in registers from the tile before:
 * there the last lead-in tile needs lead-in tiles of its own for those rows (the chunk kernel at level 10: one more; 11, 12 - chunks of
 * one row -: two more; FirstPassZW of levels 13 and 14, a row pair per tile and the pair in front of it in registers: one more) */
constexpr int lead_in_of(const bool keeps_rows, const int walk_rows) { return keeps_rows ? 1 + (2 + walk_rows - 1) / walk_rows : 1; }

// ---------------------------------------------------------------------------
// acm_tile2 with the first pass on the matrix cores, and acm_chunk: the byte-plane builds
// ---------------------------------------------------------------------------
/* [level][first pass of three / four / six stages]; the staged form differs between them (8, 16 or 64 columns of a residue class side by side).
 * Three against four: the library ships ONE of them per level, the measured better one (profiles/r4_mfma_first_pass.txt, 2.1 Gsamples per
 * level, one box: level 8 equal, level 9 three stages +1.6 %, levels 10 / 11 / 12 four stages +5.5 / +6.6 / +5 %: one LDS pass, or one of
 * its stages, less); the other depth is a tuning build (-DACM_TUNING, chosen per process with ACM_K2M_G0=3|4).
 * Six: levels whose byte-plane tiles go to the chunk kernel (acm_chunk: six stages on the matrix cores, a wavefront per chunk of 2048
 * samples) unless ACM_K3=0 asks for acm_tile2's matrix build, and - levels 13, 14 - the six-stage first pass inside acm_tile2
 * (FirstPassZW): a row pair per tile, LDS passes with barriers behind it */
struct Tile2MTile { Tile t; int lead_in; bool chunk; };         /* chunk: the chunk kernel, whose wavefronts share a launch's table among them */
#ifdef ACM_TUNING
#define ACM_GEO_ALT(...) { { __VA_ARGS__ }, 1, false }
#else
#define ACM_GEO_ALT(...) { { 0, 0, 0 }, 1, false }
#endif
#ifndef ACM_K2M_L11_TILE
#define ACM_K2M_L11_TILE 256, 8192, 4
#endif
#ifndef ACM_K2M_L12_TILE
#define ACM_K2M_L12_TILE 512, 16384, 2
#endif
#ifndef ACM_K2M_L13_TILE
#define ACM_K2M_L13_TILE 512, 16384, 2
#endif
#ifndef ACM_K3_L13_TILE
#define ACM_K3_L13_TILE 512, 16384, 2
#endif
#ifndef ACM_K3_L14_TILE
#define ACM_K3_L14_TILE 1024, 32768, 1
#endif
template <int L_>
constexpr Tile2MTile chunk_tile() { return Tile2MTile{ ChunkGeo<L_>::TILE, lead_in_of(ChunkGeo<L_>::KEEPS_ROWS, ChunkGeo<L_>::NSW), true }; }
constexpr Tile2MTile zw_tile(const int level, const Tile t) { return Tile2MTile{ t, lead_in_of(true, t.nelem >> level), false }; }
constexpr int TILE2M_G0[3] = { 3, 4, 6 };
constexpr int tile2m_slot(const int g0) { return g0 == 3 ? 0 : g0 == 4 ? 1 : 2; }
constexpr Tile2MTile TILE2M[ACM_K2M_MAX_LEVEL - ACM_K2M_MIN_LEVEL + 1][3] = {
	/* level 7: 8 residue classes of stride 8: less than one operand tile of a four-stage pass.  As a chunk kernel (two classes per row: eight
	 * row walkers per matrix set, a lane's four outputs belong to two of them) it was built, is bit-exact (tests/test_gpu_byteplane.py at the
	 * time) and SLOWER than acm_tile2's matrix build, 0.616 against 0.680: the matrix work per sample is the same at every level while the LDS
	 * passes it replaces are few at level 7.  Level 8 (four walkers): 0.680 against 0.668. */
	{ { { 256, 8192, 4 }, 1, false }, {}, {} },
	{ { { 256, 8192, 4 }, 1, false }, ACM_GEO_ALT(256, 8192, 4), chunk_tile<8>() },
	{ { { 256, 8192, 4 }, 1, false }, ACM_GEO_ALT(256, 8192, 4), chunk_tile<9>() },
	{ ACM_GEO_ALT(256, 8192, 4), { { 256, 8192, 4 }, 1, false }, chunk_tile<10>() },
	{ ACM_GEO_ALT(256, 8192, 4), { { ACM_K2M_L11_TILE }, 1, false }, chunk_tile<11>() },
	{ ACM_GEO_ALT(512, 16384, 2), { { ACM_K2M_L12_TILE }, 1, false }, chunk_tile<12>() },
	/* level 13: the vector-ALU build needs 128 KB tiles (its first pass re-runs two rows per segment); here the rows in front cost a second
	 * read through L2 and nothing else, so a tile may be one row pair.  Level 14: a row pair IS 128 KB, sixteen waves of 128 registers;
	 * (4,3,3,2,2) and (4,3,2,3,2) spill seven of them, (4,2,3,3,2) none */
	/* (level 13 as a chunk kernel: a row of 8192 per wavefront is four wavefronts of 350 registers - the staged rows of a chunk alone are
	 * 192 - and past 256 the compiler parks what the hand-issued loads have just asked for in accumulation registers BEFORE the wait,
	 * i.e. copies what is not there yet: tests/test_isa_invariants.py refuses the build.)  Levels 13 and 14: the same first pass shared
	 * by the wavefronts of a workgroup, in acm_tile2 */
	{ {}, { { ACM_K2M_L13_TILE }, 1, false }, zw_tile(13, Tile{ ACM_K3_L13_TILE }) },
	{ {}, { { 1024, 32768, 1 }, 1, false }, zw_tile(14, Tile{ ACM_K3_L14_TILE }) },
};
#undef ACM_GEO_ALT
/* the depth a level ships with where the chunk kernel / FirstPassZW is switched off (tuning builds: ACM_K3=0) */
constexpr int TILE2M_DEFAULT_G0[ACM_K2M_MAX_LEVEL - ACM_K2M_MIN_LEVEL + 1] = { 3, 3, 3, 4, 4, 4, 4, 4 };
template <int L_, int G0_>
struct Tile2MBuild : TileBuildOf<L_, TILE2M[L_ - ACM_K2M_MIN_LEVEL][tile2m_slot(G0_)].t.nt, TILE2M[L_ - ACM_K2M_MIN_LEVEL][tile2m_slot(G0_)].t.nelem,
				 TILE2M[L_ - ACM_K2M_MIN_LEVEL][tile2m_slot(G0_)].t.w> {
	static constexpr int G0 = G0_;
};

// ---------------------------------------------------------------------------
// acm_tile2p: acm_tile2 on the packed staged form
// ---------------------------------------------------------------------------
/* the tile geometries of acm_tile2 (TILE2); groups of 16 rows = one block of the usual acm_rows = 16 (level 6: 32, or a wave would hold
 * ten chunks).  (int16 only: the packed form has no float32 build) */
struct PackTile { Tile t; int gr; };
constexpr PackTile TILE2P[ACM_K2P_MAX_LEVEL - ACM_K2P_MIN_LEVEL + 1] = {
	{ { 256, 8192, 4 }, 32 }, { { 256, 8192, 4 }, 16 }, { { 256, 8192, 4 }, 16 }, { { 256, 8192, 4 }, 16 },
};
template <class C, int GR_>
struct PackGeo {
	static constexpr int GR = GR_;                          /* rows per group: one width class per column pair */
	static constexpr int NQ = GR / 4;                       /* row quads per group */
	static constexpr int RPC = 64 / NQ;                     /* column pairs (ranks) per chunk */
	static constexpr int PERMB = RPC * 2;                   /* bytes of a chunk's column-pair list */
	static constexpr int NG = C::TR / GR;
	static constexpr int P = C::COLS / 2;
	static constexpr int MAXCHUNKS = NG * (P * NQ / 64 + 3);   /* four classes per group, each rounded up to whole chunks */
	static constexpr int NW = C::NT / 64;
	static constexpr int NSLOT = (MAXCHUNKS + NW - 1) / NW; /* chunk descriptors per wave and tile */
	static constexpr int RS = C::COLS + (C::COLS >> C::PS); /* dwords between (row, c) and (row + 1, c) in the padded tile */
	static_assert(GR % 4 == 0 && 64 % NQ == 0 && C::TR % GR == 0 && (P * NQ) % 64 == 0 && PERMB % 16 == 0, "packed geometry");
	static_assert(C::COLS % (1 << C::PS) == 0, "rows are whole pad groups");
};
template <int L_>
struct Tile2PBuild : TileBuildOf<L_, TILE2P[L_ - ACM_K2P_MIN_LEVEL].t.nt, TILE2P[L_ - ACM_K2P_MIN_LEVEL].t.nelem, TILE2P[L_ - ACM_K2P_MIN_LEVEL].t.w> {
	static constexpr int GR = TILE2P[L_ - ACM_K2P_MIN_LEVEL].gr;
	using PG = PackGeo<typename Tile2PBuild::C, GR>;
	static constexpr int SLOTS = PG::NW * PG::NSLOT, PAD_SHIFT = Tile2PBuild::C::PS;
};
/* what the packed stager needs beyond the tile: chunk descriptors per tile (waves x descriptors per wave), and the pad of the tile's
 * LDS rows (one dword per 2^shift elements) */
struct PackSlots { int slots, pad_shift; };
template <int L_>
constexpr PackSlots pack_slots() { return PackSlots{ Tile2PBuild<L_>::SLOTS, Tile2PBuild<L_>::PAD_SHIFT }; }
constexpr PackSlots TILE2P_SLOTS[ACM_K2P_MAX_LEVEL - ACM_K2P_MIN_LEVEL + 1] = { pack_slots<6>(), pack_slots<7>(), pack_slots<8>(), pack_slots<9>() };

// ---------------------------------------------------------------------------
// one number over everything above
// ---------------------------------------------------------------------------
constexpr uint64_t mix(const uint64_t h, const int64_t v) { return (h ^ (uint64_t)v) * 0x100000001B3ull; }
constexpr uint64_t mix(const uint64_t h, const Tile t) { return mix(mix(mix(h, t.nt), t.nelem), t.w); }
template <int L_>
constexpr uint64_t mix_chunk(uint64_t h)
{
	using G = ChunkGeo<L_>;
	for (const int v : { G::NELEM, G::NW, G::TR, G::SIGMA, G::RR, G::NG, G::NSW, G::NX, G::NSET, G::NE, G::NM, (int)G::HISTORY_IN_REGISTERS,
			     (int)G::HISTORY_BY_DPP, (int)G::KEEPS_ROWS })
		h = mix(h, v);
	return h;
}
/* FNV-1a over every table and every ChunkGeo / PackGeo member a reader of this header can ask for */
constexpr uint64_t digest()
{
	uint64_t h = 0xCBF29CE484222325ull;
	h = mix(h, NVARIANTS);
	for (const auto &row : FUSED)
		for (const FusedTile &f : row)
			h = mix(mix(h, f.t), f.carry);
	h = mix(mix(h, PLANE.t), PLANE.carry);
	for (const Tile &t : TILE2)
		h = mix(h, t);
	for (const auto &row : TILE2M)
		for (const Tile2MTile &m : row)
			h = mix(mix(mix(h, m.t), m.lead_in), m.chunk);
	for (const int g0 : TILE2M_DEFAULT_G0)
		h = mix(h, g0);
	h = mix_chunk<12>(mix_chunk<11>(mix_chunk<10>(mix_chunk<9>(mix_chunk<8>(h)))));
	for (const PackTile &p : TILE2P)
		h = mix(mix(h, p.t), p.gr);
	for (const PackSlots &p : TILE2P_SLOTS)
		h = mix(mix(h, p.slots), p.pad_shift);
	return h;
}

} // namespace acm_geo

#endif
