/*
 * acm_kernels_tuning.inc - rows 1.. of g_fused[][] in acm_kernels.hip: the stage groupings of the alternative tile geometries behind
 * ACM_K1_VARIANT (-DACM_TUNING, profiles/sweep_variants.py; the geometries themselves: acm_kernel_geo.h, FUSED) and the timing-only
 * ablation builds of the level-7 / level-9 kernels (-DACM_ABLATION, wrong output by design).  Not part of a regular build (NVARIANTS == 1).
 */
#ifdef ACM_TUNING
	{	/* variant 1: 64 KB tiles shared by 8 waves (4 waves per SIMD, 32 elements per thread) */
		entry2<FusedBuild<1, 5>, 2, 3>(),
		entry2<FusedBuild<1, 6>, 2, 2, 2>(),
		entry2<FusedBuild<1, 7>, 2, 2, 3>(),
		entry2<FusedBuild<1, 8>, 2, 3, 3>(),
		entry2<FusedBuild<1, 9>, 2, 2, 2, 3>(),
		entry2<FusedBuild<1, 10>, 3, 3, 4>(),
		entry2<FusedBuild<1, 11>, 3, 4, 4>(),
	},
	{	/* variant 2: 128 KB tiles (one workgroup of 8 waves per CU): half the halo share of the 64 KB tiles */
		entry2<FusedBuild<2, 5>, 2, 3>(),
		entry2<FusedBuild<2, 6>, 2, 2, 2>(),
		entry2<FusedBuild<2, 7>, 2, 2, 3>(),
		entry2<FusedBuild<2, 8>, 3, 3, 2>(),
		entry2<FusedBuild<2, 9>, 3, 3, 3>(),
		entry2<FusedBuild<2, 10>, 3, 3, 4>(),
		entry2<FusedBuild<2, 11>, 3, 4, 4>(),
	},
	{	/* variant 3 */
		entry<FusedBuild<3, 5>, 2, 3>(),
		entry<FusedBuild<3, 6>, 2, 2, 2>(),
		entry<FusedBuild<3, 7>, 2, 2, 3>(),
		entry<FusedBuild<3, 8>, 2, 3, 3>(),
		entry<FusedBuild<3, 9>, 3, 3, 3>(),
		entry<FusedBuild<3, 10>, 3, 2, 2, 3>(),
		entry<FusedBuild<3, 11>, 3, 3, 2, 3>(),
	},
	{	/* variant 4 */
		entry2<FusedBuild<4, 5>, 1, 2, 2>(),
		entry2<FusedBuild<4, 6>, 2, 2, 2>(),
		entry2<FusedBuild<4, 7>, 2, 2, 3>(),
		entry2<FusedBuild<4, 8>, 3, 3, 2>(),
		entry2<FusedBuild<4, 9>, 3, 3, 3>(),
		entry2<FusedBuild<4, 10>, 3, 3, 2, 2>(),
		entry2<FusedBuild<4, 11>, 3, 3, 3, 2>(),
	},
	{	/* variant 5 */
		entry<FusedBuild<5, 5>, 3, 2>(),
		entry<FusedBuild<5, 6>, 3, 3>(),
		entry<FusedBuild<5, 7>, 3, 4>(),
		entry<FusedBuild<5, 8>, 4, 4>(),
		entry<FusedBuild<5, 9>, 3, 3, 3>(),
		entry<FusedBuild<5, 10>, 3, 3, 4>(),
		entry<FusedBuild<5, 11>, 3, 4, 4>(),
	},
	{	/* variant 6: alternative stage groupings (tuning) */
		entry2<FusedBuild<6, 5>, 1, 2, 2>(),
		entry2<FusedBuild<6, 6>, 1, 2, 3>(),
		entry2<FusedBuild<6, 7>, 1, 3, 3>(),
		entry2<FusedBuild<6, 8>, 2, 3, 3>(),
		entry2<FusedBuild<6, 9>, 2, 2, 2, 3>(),
		entry2<FusedBuild<6, 10>, 3, 2, 2, 3>(),
		entry2<FusedBuild<6, 11>, 3, 2, 3, 3>(),
	},
	{	/* variant 7: alternative stage groupings (tuning) */
		entry2<FusedBuild<7, 5>, 2, 3>(),
		entry2<FusedBuild<7, 6>, 3, 3>(),
		entry2<FusedBuild<7, 7>, 3, 2, 2>(),
		entry2<FusedBuild<7, 8>, 3, 2, 3>(),
		entry2<FusedBuild<7, 9>, 3, 2, 2, 2>(),
		entry2<FusedBuild<7, 10>, 3, 3, 4>(),
		entry2<FusedBuild<7, 11>, 3, 4, 4>(),
	},
	{	/* variant 8: 128-thread workgroups, 128 samples per thread per pass (half the warm-up share) */
		entry2<FusedBuild<8, 5>, 2, 3>(),
		entry2<FusedBuild<8, 6>, 2, 2, 2>(),
		entry2<FusedBuild<8, 7>, 2, 2, 3>(),
		entry2<FusedBuild<8, 8>, 3, 3, 2>(),
		entry2<FusedBuild<8, 9>, 3, 3, 3>(),
		entry2<FusedBuild<8, 10>, 3, 3, 4>(),
		entry2<FusedBuild<8, 11>, 3, 4, 4>(),
	},
	{	/* variant 9: 32 KB tiles, four workgroups per CU (4 waves per SIMD), carry mode */
		entry2<FusedBuild<9, 5>, 2, 3>(),
		entry2<FusedBuild<9, 6>, 2, 2, 2>(),
		entry2<FusedBuild<9, 7>, 2, 2, 3>(),
		entry2<FusedBuild<9, 8>, 3, 3, 2>(),
		entry2<FusedBuild<9, 9>, 3, 3, 3>(),
		entry2<FusedBuild<9, 10>, 3, 3, 4>(),
		entry2<FusedBuild<9, 11>, 3, 4, 4>(),
		entry2<FusedBuild<9, 12>, 3, 3, 3, 3>(),
	},
#endif
#ifdef ACM_ABLATION
	{	/* timing only: default geometry without the barriers inside the LDS passes */
		entry2<FusedBuild<10, 5>, 2, 3>(),
		entry2<FusedBuild<10, 6>, 2, 2, 2>(),
		abl2<FusedBuild<10, 7>, 32, 2, 2, 3>(),
		entry2<FusedBuild<10, 8>, 3, 3, 2>(),
		abl2<FusedBuild<10, 9>, 32, 3, 3, 3>(),
		entry2<FusedBuild<10, 10>, 3, 3, 4>(),
		entry2<FusedBuild<10, 11>, 3, 4, 4>(),
	},
	/* variants 11-19: the parts removed from levels 7 and 9 (ABL = 1, 2, 4, 6, 8, 16, 17, 23, 19), every other level as it is */
#define ACM_ABL_ROW(V, ABL) { \
		entry<FusedBuild<V, 5>, 3, 2>(), \
		entry<FusedBuild<V, 6>, 3, 3>(), \
		abl<FusedBuild<V, 7>, ABL, 3, 2, 2>(), \
		entry<FusedBuild<V, 8>, 3, 3, 2>(), \
		abl<FusedBuild<V, 9>, ABL, 3, 3, 3>(), \
		entry<FusedBuild<V, 10>, 3, 3, 2, 2>(), \
		entry<FusedBuild<V, 11>, 3, 3, 3, 2>(), \
	}
	ACM_ABL_ROW(11, 1), ACM_ABL_ROW(12, 2), ACM_ABL_ROW(13, 4), ACM_ABL_ROW(14, 6), ACM_ABL_ROW(15, 8), ACM_ABL_ROW(16, 16), ACM_ABL_ROW(17, 17),
	ACM_ABL_ROW(18, 23), ACM_ABL_ROW(19, 19),
#undef ACM_ABL_ROW
#endif
