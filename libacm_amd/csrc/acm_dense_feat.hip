/*
 * acm_dense_feat.hip - the two launches acm_batch_decode_windows_features (acm_batch_windows.cpp) puts behind the overlay's combine
 * launch: mel filterbank features of the int16 rows that launch wrote into the feature arena, defined on integers
 * (include/acm_hip.h) and computed on the matrix cores.  No counterpart in the reference.
 *
 * The DFT of 16 frames at a time is a 16 x N by N x 16 product per tile of 16 columns, and v_mfma_i32_16x16x64_i8 gives it exactly
 * when both operands are split into signed bytes, v = 256 hi + lo (acm_feat_layout.h; FirstPassZ of acm_kernels.hip does the same
 * with the synthesis filters): four products per tile and K step - hi.hi, hi.lo, lo.hi, lo.lo - into four int32 accumulators, every
 * partial sum below 2^26, joined in 64 bits behind the last K step.
 *
 * Operand maps (v_mfma_i32_16x16x64_i8, 16 bytes of A and of B per lane; acm_kernels.hip has them at FirstPassM / FirstPassZ): lane
 * l holds A[row l % 16][k = 16 (l / 16) + j] and B[k = 16 (l / 16) + j][column l % 16] in byte j, and receives D[row 4 (l / 16) +
 * reg][column l % 16] in register reg < 4.  Rows are frames, k is the sample of the frame, columns are bins.
 *
 * acm_feat_twiddle  builds the B operand from c[]: per bin tile bt < N / 32 + 1 a tile of cosine columns (bins 16 bt .. 16 bt + 15)
 *                   and a tile of sine columns, per K step a hi and a lo plane of 64 lanes x 16 bytes, in that order - so a wavefront
 *                   reads a plane as one coalesced KB, and Re and Im of one (frame, bin) land in the same lane.  Columns of bins
 *                   past N / 2 are zero.  One thread per lane's 16 bytes of both planes; the host loops over nothing.
 * acm_dense_feat    a workgroup of four wavefronts per (row, tile of 16 frames), the grid capped and strided over like every dense
 *                   kernel's.  The span of the row under the 16 frames is put into LDS once, zeros outside [0, T) by a clamped
 *                   address and a select, no branch; the frames are windowed and split into hi and lo planes in LDS in A-operand
 *                   order (rows padded by 16 bytes, which takes the 16 frames of a ds_read_b128 off each other's banks).  Then,
 *                   four bin tiles at a time, one per wavefront: N / 64 K steps of 8 matrix instructions, Re, Im, the shift, the
 *                   squares and P as two 32-bit limbs into 2 KB of LDS per wavefront; behind a barrier all 256 lanes run the mel
 *                   stage over those 64 bins - a lane owns one frame and up to 8 bands and adds w * P_hi and w * P_lo to two
 *                   uint64 sums per band, both below 2^58 - so P of all bins is never resident.  trunc24 and the store end the
 *                   item: lanes along f for the default layout, along b for ACM_FEAT_TIME_MAJOR.  Built three times over: for
 *                   acm_batch_decode_windows_logmel the item ends with the integer logarithm of the sums instead
 *                   (acm_feat_log_q16), scaled to the final float, or - with ACM_FEAT_LOG_TOP - stored as it is, its maximum over
 *                   the wavefront going into the row's entry of a table with one vector atomic.
 * acm_feat_log_finish  behind such a launch: every word of the tensor once more, in place - the clamp to the row's maximum, the scale,
 *                   the float.
 */
#include <hip/hip_runtime.h>

#include "acm_dense_vec.h"
#include "acm_device.h"
#include "acm_feat_layout.h"

namespace {

constexpr int FEAT_BLOCK = 256;                         /* four wavefronts */
constexpr int FEAT_WAVES = FEAT_BLOCK / 64;
constexpr int FEAT_TILE = ACM_FEAT_TILE;
constexpr int FEAT_KSTEP = ACM_FEAT_KSTEP;
constexpr int FEAT_BANDS_PER_LANE = ACM_FEAT_MAX_MELS / 16;
constexpr int FEAT_ROW_PAD = 16;                        /* bytes behind a frame's N bytes of a plane */
constexpr int FEAT_PBUF_BYTES = FEAT_WAVES * 16 * FEAT_TILE * 8;

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(FEAT_BLOCK) void acm_feat_twiddle(const int16_t *__restrict__ cs, uint32_t n_fft, uint32_t ksteps, uint32_t nthreads,
								i32x4 *__restrict__ tw)
{
	const uint32_t g = blockIdx.x * FEAT_BLOCK + threadIdx.x;
	if (g >= nthreads)
		return;
	const uint32_t lane = g & 63u, blk = g >> 6;            /* blk = (bt * 2 + part) * ksteps + ks */
	const uint32_t ks = blk % ksteps, part = (blk / ksteps) & 1u, bt = blk / ksteps / 2;
	const uint32_t bin = bt * 16 + (lane & 15u), t0 = ks * FEAT_KSTEP + (lane >> 4) * 16;
	const uint32_t phase = part ? 3 * n_fft / 4 : 0;
	uint32_t hi[4] = {}, lo[4] = {};
#pragma unroll
	for (uint32_t j = 0; j < 16; j++) {
		const int v = bin <= n_fft / 2 ? (int)cs[(bin * (t0 + j) + phase) & (n_fft - 1)] : 0;
		hi[j / 4] |= ((uint32_t)acm_feat_hi(v) & 0xFFu) << (8 * (j % 4));
		lo[j / 4] |= ((uint32_t)acm_feat_lo(v) & 0xFFu) << (8 * (j % 4));
	}
	i32x4 *at = tw + (size_t)blk * 128 + lane;
	at[0] = i32x4{ (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3] };
	at[64] = i32x4{ (int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3] };
}

/* what the feature kernel ends an item with: the linear feature (acm_batch_decode_windows_features); of
 * acm_batch_decode_windows_logmel the final float, or with ACM_FEAT_LOG_TOP L itself and the row's maximum */
enum { FEAT_LINEAR = 0, FEAT_LOG = 1, FEAT_LOG_TOP = 2 };

/* N: n_fft; TM: ACM_FEAT_TIME_MAJOR; LOG: FEAT_* */
template <int N, bool TM, int LOG>
__global__ __launch_bounds__(FEAT_BLOCK) void acm_dense_feat(const int16_t *__restrict__ rows, const AcmFeatDesc d, uint32_t *__restrict__ out, uint64_t T,
							      uint64_t F, uint64_t tiles, uint64_t nwork)
{
	constexpr int KS = N / FEAT_KSTEP, NBT = N / 32 + 1, NG = (NBT + FEAT_WAVES - 1) / FEAT_WAVES, BINS = N / 2 + 1;
	constexpr int ROWB = N + FEAT_ROW_PAD, PLANE = FEAT_TILE * ROWB;
	constexpr int SPAN_BYTES = 2 * FEAT_TILE * N;           /* 15 hops and a frame, at hop == N */
	constexpr int SHARED = SPAN_BYTES > FEAT_PBUF_BYTES ? SPAN_BYTES : FEAT_PBUF_BYTES;
	constexpr uint32_t LOG2N = N == 128 ? 7 : N == 256 ? 8 : N == 512 ? 9 : N == 1024 ? 10 : 11;
	/* one array: the hi plane, the lo plane, and behind them the span, which P of four bin tiles takes over once the planes are made */
	__shared__ __attribute__((aligned(16))) uint8_t lds[2 * PLANE + SHARED];
	uint8_t *const plane_hi = lds, *const plane_lo = lds + PLANE;
	int16_t *const span = reinterpret_cast<int16_t *>(lds + 2 * PLANE);
	uint64_t *const pbuf = reinterpret_cast<uint64_t *>(lds + 2 * PLANE);

	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t H = d.hop, B = d.n_mels;
	const int64_t pad = (d.flags & ACM_FEAT_CENTER) ? N / 2 : 0;
	const uint32_t span_len = (FEAT_TILE - 1) * H + N;
	/* the mel stage's lane: one frame of the tile and bands bl, bl + 16, ... */
	const uint32_t mf = TM ? tid >> 4 : tid & 15u, bl = TM ? tid & 15u : tid >> 4;
	uint32_t m_first[FEAT_BANDS_PER_LANE], m_end[FEAT_BANDS_PER_LANE], m_off[FEAT_BANDS_PER_LANE];
#pragma unroll
	for (int j = 0; j < FEAT_BANDS_PER_LANE; j++) {
		const uint32_t b = bl + 16 * j;
		const bool live = b < B;
		const uint32_t bc = live ? b : 0;               /* a band the bank has: nothing is read behind the tables */
		m_first[j] = d.mel_first[bc];
		m_end[j] = live ? m_first[j] + d.mel_count[bc] : m_first[j];
		m_off[j] = d.mel_off[bc];
	}

	for (uint64_t work = blockIdx.x; work < nwork; work += gridDim.x) {
		const uint64_t r = work / tiles, f0 = (work - r * tiles) * FEAT_TILE;
		const int16_t *x = rows + r * T;
		const int64_t s0 = (int64_t)(f0 * H) - pad;     /* the sample of the row at place 0 of the span */
		__syncthreads();                                /* the item before this one has read its last P */
		for (uint32_t i = tid; i < span_len; i += FEAT_BLOCK) {
			const int64_t at = s0 + i, c = at < 0 ? 0 : at >= (int64_t)T ? (int64_t)T - 1 : at;
			const int16_t v = x[c];
			span[i] = c == at ? v : (int16_t)0;
		}
		__syncthreads();
		for (uint32_t u = tid; u < FEAT_TILE * N / 4; u += FEAT_BLOCK) {
			const uint32_t f = u / (N / 4), t = (u % (N / 4)) * 4;
			const uint2 w2 = *reinterpret_cast<const uint2 *>(d.window + t);
			const int w[4] = { (int)(w2.x & 0xFFFFu), (int)(w2.x >> 16), (int)(w2.y & 0xFFFFu), (int)(w2.y >> 16) };
			uint32_t hi = 0, lo = 0;
#pragma unroll
			for (int e = 0; e < 4; e++) {
				const int xw = ((int)span[f * H + t + e] * w[e] + 16384) >> 15;
				hi |= ((uint32_t)acm_feat_hi(xw) & 0xFFu) << (8 * e);
				lo |= ((uint32_t)acm_feat_lo(xw) & 0xFFu) << (8 * e);
			}
			*reinterpret_cast<uint32_t *>(plane_hi + f * ROWB + t) = hi;
			*reinterpret_cast<uint32_t *>(plane_lo + f * ROWB + t) = lo;
		}
		__syncthreads();

		uint64_t e_hi[FEAT_BANDS_PER_LANE] = {}, e_lo[FEAT_BANDS_PER_LANE] = {};
		for (int g = 0; g < NG; g++) {
			const uint32_t bt = g * FEAT_WAVES + wave;
			if (bt < NBT) {
				const i32x4 zero = { 0, 0, 0, 0 };
				i32x4 re_hh = zero, re_hl = zero, re_lh = zero, re_ll = zero, im_hh = zero, im_hl = zero, im_lh = zero, im_ll = zero;
				const i32x4 *bp = reinterpret_cast<const i32x4 *>(d.twiddle) + (size_t)bt * (2 * KS * 128) + lane;
				const uint8_t *ap = plane_hi + (lane & 15u) * ROWB + (lane >> 4) * 16;
#pragma unroll 2
				for (int ks = 0; ks < KS; ks++) {
					const i32x4 a_hi = *reinterpret_cast<const i32x4 *>(ap + ks * FEAT_KSTEP);
					const i32x4 a_lo = *reinterpret_cast<const i32x4 *>(ap + PLANE + ks * FEAT_KSTEP);
					const i32x4 c_hi = bp[ks * 128], c_lo = bp[ks * 128 + 64];
					const i32x4 s_hi = bp[(KS + ks) * 128], s_lo = bp[(KS + ks) * 128 + 64];
					re_hh = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_hi, c_hi, re_hh, 0, 0, 0);
					re_hl = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_hi, c_lo, re_hl, 0, 0, 0);
					re_lh = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_lo, c_hi, re_lh, 0, 0, 0);
					re_ll = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_lo, c_lo, re_ll, 0, 0, 0);
					im_hh = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_hi, s_hi, im_hh, 0, 0, 0);
					im_hl = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_hi, s_lo, im_hl, 0, 0, 0);
					im_lh = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_lo, s_hi, im_lh, 0, 0, 0);
					im_ll = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_lo, s_lo, im_ll, 0, 0, 0);
				}
				/* register j: frame 4 (lane / 16) + j, bin 16 bt + lane % 16; P[wave][bin % 16][frame] */
				uint64_t *pw = pbuf + (wave * 16 + (lane & 15u)) * FEAT_TILE + (lane >> 4) * 4;
#pragma unroll
				for (int j = 0; j < 4; j++) {
					const int64_t a = acm_feat_scale(acm_feat_join(re_hh[j], re_hl[j], re_lh[j], re_ll[j]), LOG2N);
					const int64_t bv = acm_feat_scale(-acm_feat_join(im_hh[j], im_hl[j], im_lh[j], im_ll[j]), LOG2N);
					pw[j] = (uint64_t)(a * a) + (uint64_t)(bv * bv);
				}
			}
			__syncthreads();
			const uint32_t k0 = (uint32_t)g * (FEAT_WAVES * 16), k1 = k0 + FEAT_WAVES * 16;
#pragma unroll
			for (int j = 0; j < FEAT_BANDS_PER_LANE; j++) {
				const uint32_t lo = m_first[j] > k0 ? m_first[j] : k0, hi = m_end[j] < k1 ? m_end[j] : k1;
				for (uint32_t k = lo; k < hi; k++) {
					const uint64_t p = pbuf[(k - k0) * FEAT_TILE + mf];
					const uint64_t w = d.mel_w[m_off[j] + (k - m_first[j])];
					e_hi[j] += w * (p >> 32);
					e_lo[j] += w * (p & 0xFFFFFFFFull);
				}
			}
			__syncthreads();
		}
		static_assert(NG * FEAT_WAVES * 16 >= BINS, "the groups of bin tiles cover every bin");

		const uint64_t frame = f0 + mf;
		int32_t top = INT32_MIN;                        /* of this lane's L: below every floor */
		if (frame < F) {
#pragma unroll
			for (int j = 0; j < FEAT_BANDS_PER_LANE; j++) {
				const uint32_t b = bl + 16 * j;
				if (b < B) {
					uint32_t v;
					if (LOG == FEAT_LINEAR) {
						v = acm_feat_trunc24_bits(e_hi[j], e_lo[j], LOG2N);
					} else {
						const int32_t l = acm_feat_log_q16(e_hi[j], e_lo[j], LOG2N, d.floor_q16);
						top = l > top ? l : top;
						v = LOG == FEAT_LOG_TOP ? (uint32_t)l : acm_feat_log_out(l, d.mul_q24, d.offset_q16);
					}
					out[TM ? (r * F + frame) * B + b : (r * B + b) * F + frame] = v;
				}
			}
		}
		if (LOG == FEAT_LOG_TOP) {
			/* the item is of one row: the wavefront's maximum, then one vector atomic of its first lane */
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) {
				const int32_t other = __shfl_xor(top, o, 64);
				top = other > top ? other : top;
			}
			if (lane == 0 && top != INT32_MIN)
				atomicMax(d.rowmax + r, top);
		}
	}
}

/* the second pass of a call with ACM_FEAT_LOG_TOP, in place over the tensor's words: L clamped to its row's maximum less top_q16,
 * scaled, as a float.  One dword per lane and trip - the tensor may start anywhere on a multiple of 4 - and the grid strides */
__global__ __launch_bounds__(FEAT_BLOCK) void acm_feat_log_finish(uint32_t *__restrict__ out, const int32_t *__restrict__ rowmax, uint64_t total,
								   uint64_t per_row, int32_t top_q16, uint32_t mul_q24, int32_t offset_q16)
{
	for (uint64_t i = (uint64_t)blockIdx.x * FEAT_BLOCK + threadIdx.x; i < total; i += (uint64_t)gridDim.x * FEAT_BLOCK) {
		const int32_t l = (int32_t)out[i], least = rowmax[i / per_row] - top_q16;
		out[i] = acm_feat_log_out(l > least ? l : least, mul_q24, offset_q16);
	}
}

template <int N, int LOG>
int launch_feat(bool tm, dim3 grid, hipStream_t st, const int16_t *rows, const AcmFeatDesc &d, uint32_t *out, uint64_t T, uint64_t F, uint64_t tiles, uint64_t nwork)
{
	if (tm)
		hipLaunchKernelGGL((acm_dense_feat<N, true, LOG>), grid, dim3(FEAT_BLOCK), 0, st, rows, d, out, T, F, tiles, nwork);
	else
		hipLaunchKernelGGL((acm_dense_feat<N, false, LOG>), grid, dim3(FEAT_BLOCK), 0, st, rows, d, out, T, F, tiles, nwork);
	return (int)hipGetLastError();
}

/* the feature launch of either entry point: the geometry, the refusals and the choice of the transform's build */
template <int LOG>
int launch_dense_feat(const int16_t *d_rows, uint64_t nrows, uint64_t frames, const AcmFeatDesc &d, uint32_t *out, uint32_t dense_grid, hipStream_t st)
{
	if (d.hop == 0 || d.hop > d.n_fft || d.n_mels == 0 || d.n_mels > ACM_FEAT_MAX_MELS || frames == 0 || frames > (1ull << 40))
		return (int)hipErrorInvalidValue;
	const uint64_t F = (d.flags & ACM_FEAT_CENTER) ? 1 + frames / d.hop : frames >= d.n_fft ? 1 + (frames - d.n_fft) / d.hop : 0;
	const AcmFeatGeo g = acm_feat_geo(nrows, F, dense_grid, DENSE_MAX_GRID);
	if (!g.ok)
		return (int)hipErrorInvalidValue;
	if (g.nwork == 0)
		return 0;
	const bool tm = (d.flags & ACM_FEAT_TIME_MAJOR) != 0;
	switch (d.n_fft) {
	case 128:
		return launch_feat<128, LOG>(tm, dim3(g.grid), st, d_rows, d, out, frames, F, g.tiles, g.nwork);
	case 256:
		return launch_feat<256, LOG>(tm, dim3(g.grid), st, d_rows, d, out, frames, F, g.tiles, g.nwork);
	case 512:
		return launch_feat<512, LOG>(tm, dim3(g.grid), st, d_rows, d, out, frames, F, g.tiles, g.nwork);
	case 1024:
		return launch_feat<1024, LOG>(tm, dim3(g.grid), st, d_rows, d, out, frames, F, g.tiles, g.nwork);
	case 2048:
		return launch_feat<2048, LOG>(tm, dim3(g.grid), st, d_rows, d, out, frames, F, g.tiles, g.nwork);
	default:
		return (int)hipErrorInvalidValue;
	}
}

} // namespace

extern "C" int acmk_launch_feat_twiddle(const int16_t *d_cs, uint32_t n_fft, void *d_twiddle, void *stream)
{
	if (n_fft < ACM_FEAT_MIN_FFT || n_fft > ACM_FEAT_MAX_FFT || (n_fft & (n_fft - 1)) != 0)
		return (int)hipErrorInvalidValue;
	const uint32_t ksteps = n_fft / FEAT_KSTEP, nthreads = acm_feat_bin_tiles(n_fft) * 2 * ksteps * 64;
	hipLaunchKernelGGL(acm_feat_twiddle, dim3((nthreads + FEAT_BLOCK - 1) / FEAT_BLOCK), dim3(FEAT_BLOCK), 0, (hipStream_t)stream, d_cs, n_fft, ksteps,
			   nthreads, static_cast<i32x4 *>(d_twiddle));
	return (int)hipGetLastError();
}

extern "C" int acmk_launch_dense_feat(const int16_t *d_rows, uint64_t nrows, uint64_t frames, const AcmFeatDesc *desc, float *d_out, uint32_t dense_grid,
				      void *stream)
{
	return launch_dense_feat<FEAT_LINEAR>(d_rows, nrows, frames, *desc, reinterpret_cast<uint32_t *>(d_out), dense_grid, (hipStream_t)stream);
}

extern "C" int acmk_launch_feat_log_finish(float *d_out, uint64_t total, uint64_t per_row, const AcmFeatDesc *desc, uint32_t dense_grid, void *stream)
{
	if (total == 0)
		return 0;
	if (per_row == 0 || !desc->rowmax || desc->top_q16 > ACM_FEAT_LOG_TOP_MAX)
		return (int)hipErrorInvalidValue;
	const uint64_t blocks = (total + FEAT_BLOCK - 1) / FEAT_BLOCK;
	const uint32_t cap = acm_cap_value(dense_grid, DENSE_MAX_GRID);
	hipLaunchKernelGGL(acm_feat_log_finish, dim3((uint32_t)(blocks < cap ? blocks : cap)), dim3(FEAT_BLOCK), 0, (hipStream_t)stream,
			   reinterpret_cast<uint32_t *>(d_out), desc->rowmax, total, per_row, (int32_t)desc->top_q16, desc->mul_q24, desc->offset_q16);
	return (int)hipGetLastError();
}

extern "C" int acmk_launch_dense_logmel(const int16_t *d_rows, uint64_t nrows, uint64_t frames, const AcmFeatDesc *desc, float *d_out, uint32_t dense_grid,
					void *stream)
{
	const AcmFeatDesc &d = *desc;
	const hipStream_t st = (hipStream_t)stream;
	uint32_t *out = reinterpret_cast<uint32_t *>(d_out);
	if (!(d.log_flags & ACM_FEAT_LOG_TOP))
		return launch_dense_feat<FEAT_LOG>(d_rows, nrows, frames, d, out, dense_grid, st);
	if (!d.rowmax)
		return (int)hipErrorInvalidValue;
	/* every byte 0x80: an int32 below every L, so a maximum left by the call before never shows */
	int e = nrows ? (int)hipMemsetAsync(d.rowmax, 0x80, nrows * sizeof(int32_t), st) : 0;
	if (e == 0)
		e = launch_dense_feat<FEAT_LOG_TOP>(d_rows, nrows, frames, d, out, dense_grid, st);
	if (e != 0)
		return e;
	const uint64_t F = (d.flags & ACM_FEAT_CENTER) ? 1 + frames / d.hop : frames >= d.n_fft ? 1 + (frames - d.n_fft) / d.hop : 0;
	return acmk_launch_feat_log_finish(d_out, nrows * d.n_mels * F, (uint64_t)d.n_mels * F, desc, dense_grid, stream);
}
