/*
 * acm_dense_fir.hip - the launch acm_batch_decode_windows_overlay_fir (acm_batch_windows.cpp) puts between a dense call's gather launch
 * and the overlay's energy launch: source rows convolved with an impulse response (include/acm_hip.h), channel by channel, into rows
 * of their own behind the source rows of the same arena (acm_fir_layout.h).
 *
 * No counterpart in the reference.  A flat grid over (filtered row, channel, tile) on the dense kernels' unit (acm_dense_geo.h: 256
 * lanes, 8 outputs a lane, 2048 outputs a tile).  The response comes reversed and zero-padded to whole tap blocks of 64
 * (acm_fir_layout.cpp), so y[j] = sum over u of g[u] * x[j + lead + u] reads both operands upwards, two at a time:
 *
 *   taps      wave-uniform: 32 dwords of tap pairs per block, read through the scalar cache into SGPRs - no vector or LDS traffic
 *   input     a stage - the tile's 2048 samples and up to 8 tap blocks more, 5120 bytes - is put into LDS once, one channel's samples
 *             in order (this is where an interleaved row is de-interleaved), zeros outside [0, T); a stage wholly outside is skipped
 *   a lane    reads 36 dwords of it per tap block as 9 ds_read_b128 (lane l at byte 16 l: no bank conflict), which are the even-aligned
 *             pairs of its 8 outputs' windows; one alignment (v_perm) per dword makes the odd-aligned ones.  Then 8 v_dot2c_i32_i16 per
 *             tap pair with the pair as the scalar operand: 16 multiply-adds for 8 vector instructions, and 37 others per block
 *   sums      int32, exact: sum |h| <= 65535 (acm_dense_fir_check) bounds every partial sum by 65535 * 32768 < 2^31
 *
 * Tiles are cut where the DESTINATION sub-row's aligned 16-byte lines are (planar and mono), so every lane whose 8 outputs lie inside
 * the row stores one whole line; the up to 7 outputs in front of the first line and behind the last are single stores of the first
 * and the last vector.  An interleaved row's channel is every second element: single stores throughout.
 */
#include <hip/hip_runtime.h>

#include "acm_dense_vec.h"
#include "acm_device.h"

namespace {

constexpr int FIR_TB = ACM_FIR_TAP_BLOCK;               /* taps of a block: 32 SGPRs of pairs */
constexpr int FIR_STAGE_BLOCKS = 8;                     /* tap blocks a stage of LDS serves */
constexpr int FIR_LDS_SAMPLES = DENSE_UNIT + FIR_STAGE_BLOCKS * FIR_TB;
constexpr int FIR_DW = FIR_TB / 2 + 4;                  /* dwords of LDS a lane reads per tap block: 8 outputs' windows over 64 taps */

typedef short s16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int dot2(uint32_t x, uint32_t g, int acc)
{
	return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, x), __builtin_bit_cast(s16x2, g), acc, false);
}

/* STRIDE: elements between a channel's consecutive frames - 1 (mono, a plane), 2 (interleaved stereo) */
template <int STRIDE>
__global__ __launch_bounds__(DENSE_BLOCK) void acm_dense_fir(int16_t *__restrict__ src, const AcmFirRow *__restrict__ rows, const uint32_t *__restrict__ taps,
							      uint64_t nwork, uint32_t units, uint32_t channels, int64_t frames, uint64_t row_len)
{
	__shared__ u32x4 seg[FIR_LDS_SAMPLES / 8];
	uint32_t *seg32 = reinterpret_cast<uint32_t *>(seg);
	for (uint64_t work = blockIdx.x; work < nwork; work += gridDim.x) {
		const uint64_t rc = work / units;
		const uint32_t unit = (uint32_t)(work - rc * units);
		const uint64_t i = rc / channels;
		const uint32_t ch = (uint32_t)(rc - i * channels);
		const AcmFirRow row = rows[i];
		const uint64_t sub = STRIDE == 1 ? (uint64_t)ch * (uint64_t)frames : ch;
		const int16_t *x = src + (uint64_t)row.src * row_len + sub;
		int16_t *y = src + (uint64_t)row.dst * row_len + sub;
		/* output 0 lies this far into its aligned line: the tiles begin at that line */
		const int64_t org = STRIDE == 1 ? -(int64_t)(line_shift(y) / sizeof(int16_t)) : 0;
		const int64_t j0 = org + (int64_t)unit * DENSE_UNIT;
		if (j0 >= frames)               /* the geometry counts the up to 7 places in front of output 0 in: the last tile can be empty */
			continue;
		int acc[DENSE_VEC] = {};
		for (uint32_t kb0 = 0; kb0 < row.nblk; kb0 += FIR_STAGE_BLOCKS) {
			const uint32_t nb = row.nblk - kb0 < (uint32_t)FIR_STAGE_BLOCKS ? row.nblk - kb0 : (uint32_t)FIR_STAGE_BLOCKS;
			const uint32_t nstage = DENSE_UNIT + nb * FIR_TB;
			const int64_t s0 = j0 + row.lead + (int64_t)kb0 * FIR_TB;       /* the sample of x at place 0 of the stage */
			if (s0 >= frames || s0 + (int64_t)nstage <= 0)                  /* zeros alone: the workgroup's branch */
				continue;
			__syncthreads();                /* the stage before this one has been read */
			for (uint32_t q = threadIdx.x; q < nstage / 2; q += DENSE_BLOCK) {
				const int64_t i0 = s0 + 2 * (int64_t)q, i1 = i0 + 1;
				/* both loads at a place inside the row, without a branch; what lies outside is zero */
				const int64_t c0 = i0 < 0 ? 0 : i0 >= frames ? frames - 1 : i0, c1 = i1 < 0 ? 0 : i1 >= frames ? frames - 1 : i1;
				const uint32_t lo = (uint16_t)x[c0 * STRIDE], hi = (uint16_t)x[c1 * STRIDE];
				seg32[q] = (c0 == i0 ? lo : 0u) | (c1 == i1 ? hi : 0u) << 16;
			}
			__syncthreads();
			for (uint32_t kb = 0; kb < nb; kb++) {
				const uint32_t *tp = taps + row.taps_off + (uint64_t)(kb0 + kb) * (FIR_TB / 2);
				const u32x4 *xp = seg + threadIdx.x + kb * (FIR_TB / 8);
				uint32_t d[FIR_DW];
#pragma unroll
				for (int v = 0; v < FIR_DW / 4; v++) {
					const u32x4 t = xp[v];
					d[4 * v] = t.x;
					d[4 * v + 1] = t.y;
					d[4 * v + 2] = t.z;
					d[4 * v + 3] = t.w;
				}
#pragma unroll
				for (int p = 0; p < FIR_TB / 2; p++) {
					const uint32_t g = tp[p];
#pragma unroll
					for (int e = 0; e < DENSE_VEC / 2; e++) {
						acc[2 * e] = dot2(d[e + p], g, acc[2 * e]);
						acc[2 * e + 1] = dot2(__builtin_amdgcn_alignbit(d[e + p + 1], d[e + p], 16), g, acc[2 * e + 1]);
					}
				}
			}
		}
		const long long half = row.shift ? 1ll << (row.shift - 1) : 0;
		int s[DENSE_VEC];
#pragma unroll
		for (int o = 0; o < DENSE_VEC; o++) {
			const long long v = (acc[o] + half) >> row.shift;
			s[o] = v < -32768 ? -32768 : v > 32767 ? 32767 : (int)v;
		}
		const int64_t j = j0 + (int64_t)threadIdx.x * DENSE_VEC;
		if (STRIDE == 1 && j >= 0 && j + DENSE_VEC <= frames) {
			store_vec<false>(y + j, s);
		} else {
#pragma unroll
			for (int o = 0; o < DENSE_VEC; o++)
				if (j + o >= 0 && j + o < frames)
					y[(j + o) * STRIDE] = (int16_t)s[o];
		}
	}
}

} // namespace

extern "C" int acmk_launch_dense_fir(int16_t *d_src, const AcmFirRow *d_rows, uint64_t nfilt, const uint32_t *d_taps, uint64_t frames, uint32_t channels,
				     int planar, uint32_t dense_grid, void *stream)
{
	if (nfilt == 0 || frames == 0 || channels == 0)
		return 0;
	if (channels > 2 || nfilt > ~0ull / channels || frames > (1ull << 40))
		return (int)hipErrorInvalidValue;
	/* a "row" of the geometry is one channel of one filtered row: its frames and the up to 7 places in front of its first aligned
	 * line, in whole vectors */
	const DenseGeo g = dense_geo(nfilt * channels, frames + (DENSE_VEC - 1), 1, 0, dense_grid, DENSE_MAX_GRID, true);
	if (!g.ok)
		return (int)hipErrorInvalidValue;
	const uint64_t row_len = frames * channels;
	if (channels == 2 && !planar)
		hipLaunchKernelGGL(acm_dense_fir<2>, dim3(g.grid), dim3(DENSE_BLOCK), 0, (hipStream_t)stream, d_src, d_rows, d_taps, g.nwork, g.units, channels,
				   (int64_t)frames, row_len);
	else
		hipLaunchKernelGGL(acm_dense_fir<1>, dim3(g.grid), dim3(DENSE_BLOCK), 0, (hipStream_t)stream, d_src, d_rows, d_taps, g.nwork, g.units, channels,
				   (int64_t)frames, row_len);
	return (int)hipGetLastError();
}
