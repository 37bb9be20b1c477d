/*
 * acm_feat_layout.h - the device-free half of acm_batch_decode_windows_features (acm_batch_windows.cpp): whether the bank is one the
 * call takes (acm_feat_bank_check, the one text of it), the designed tables (acm_feat_design), the frame count, the byte split of the
 * DFT's operands, the join of the four matrix products, the two-limb mel sum's end (trunc24), the geometry of the feature grid and
 * the sizes of what is uploaded and of the feature arena; and of acm_batch_decode_windows_logmel: the integer logarithm of that sum
 * (acm_feat_log_q16), its scale (acm_feat_log_out), the check of both (acm_feat_log_check) and the rows' maxima.  Internal.  Neither this header nor acm_feat_layout.cpp knows a device
 * (tests/test_dense_feat.py, tests/native/feat_layout.cpp); what is marked ACM_FEAT_HD is compiled into the kernels
 * (acm_dense_feat.hip) too, so the program without a device checks the text the device runs.
 */
#ifndef ACM_FEAT_LAYOUT_H
#define ACM_FEAT_LAYOUT_H

#include <stddef.h>
#include <stdint.h>

#include "acm_hip.h"
#include "acm_launch_caps.h"

#ifdef __HIP__
#define ACM_FEAT_HD __host__ __device__
#else
#define ACM_FEAT_HD
#endif

#define ACM_FEAT_TILE 16u                       /* frames of a workgroup: the rows of one matrix instruction */
#define ACM_FEAT_KSTEP 64u                      /* samples of a frame one v_mfma_i32_16x16x64_i8 sums over */
#define ACM_FEAT_MIN_FFT 128u
#define ACM_FEAT_MAX_FFT 2048u
#define ACM_FEAT_ROW_SLACK 64u                  /* int16 samples the arena is asked for behind the last row */

/* v = 256 * hi + lo with lo the signed low byte: for |v| <= 32639 both are int8, and for |v| <= 16384 |hi| <= 64 */
ACM_FEAT_HD static inline int acm_feat_lo(int v) { return (int)(int8_t)(uint8_t)((unsigned)v & 0xFFu); }
ACM_FEAT_HD static inline int acm_feat_hi(int v) { return (v - acm_feat_lo(v)) >> 8; }

/* sum x * c from the four products of the byte planes (x = 256 xh + xl, c = 256 ch + cl): HH = sum xh * ch, HL = sum xh * cl,
 * LH = sum xl * ch, LL = sum xl * cl.  Each is below 2^26 in magnitude at N = 2048 (|xh| <= 127, |ch| <= 64, |xl|, |cl| <= 128) */
ACM_FEAT_HD static inline int64_t acm_feat_join(int32_t hh, int32_t hl, int32_t lh, int32_t ll)
{
	return (int64_t)hh * 65536 + ((int64_t)hl + (int64_t)lh) * 256 + (int64_t)ll;
}

/* A of include/acm_hip.h from Re (or Bv from Im): q = n - 1 >= 6 */
ACM_FEAT_HD static inline int64_t acm_feat_scale(int64_t re, uint32_t n) { return (re + ((int64_t)1 << (n - 2))) >> (n - 1); }

/* E = s_hi * 2^32 + s_lo from the two limb sums of a band (s_hi = sum w * (P >> 32), s_lo = sum w * (P mod 2^32), both below 2^58):
 * the position p of its leading bit, - 1 for E = 0, and *m in [2^23, 2^24) its 24 leading bits (shifted left for p < 23) */
ACM_FEAT_HD static inline int acm_feat_lead(uint64_t s_hi, uint64_t s_lo, uint32_t *m)
{
	const uint64_t lo = (s_hi << 32) + s_lo;
	const uint64_t hi = (s_hi >> 32) + (lo < s_lo ? 1u : 0u);
	*m = 0;
	if ((hi | lo) == 0)
		return -1;
	const int p = hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo);        /* the leading bit of E */
	if (p <= 23) {
		*m = (uint32_t)(lo << (23 - p));                                        /* ... at bit 23 of m */
	} else {
		const int sh = p - 23;
		*m = (uint32_t)(sh >= 64 ? hi >> (sh - 64) : (lo >> sh) | (hi ? hi << (64 - sh) : 0)) & 0xFFFFFFu;
	}
	return p;
}

/* y of include/acm_hip.h from the two limb sums: the 24 leading bits of E, as a float32 with exponent - (75 - 2 n).  Nothing is
 * rounded; E = 0 is +0.0 */
ACM_FEAT_HD static inline uint32_t acm_feat_trunc24_bits(uint64_t s_hi, uint64_t s_lo, uint32_t n)
{
	uint32_t m;
	const int p = acm_feat_lead(s_hi, s_lo, &m);
	if (p < 0)
		return 0;
	const int e = p - (75 - 2 * (int)n);
	return (uint32_t)(e + 127) << 23 | (m & 0x7FFFFFu);
}

/* frac of include/acm_hip.h: the sixteen bits behind the point of log2(m / 2^23), m in [2^23, 2^24), by sixteen squarings - the
 * square of x in [2^23, 2^24) is in [2^46, 2^48), its bit 47 is the next bit of the logarithm, and the shift keeps x in range */
ACM_FEAT_HD static inline uint32_t acm_feat_log_frac(uint32_t m)
{
	uint64_t x = m;
	uint32_t frac = 0;
	for (int i = 0; i < 16; i++) {
		x *= x;
		const uint32_t bit = (uint32_t)(x >> 47);
		x >>= 23 + bit;
		frac = frac << 1 | bit;
	}
	return frac;
}

/* L of include/acm_hip.h from the two limb sums: log2 of y in Q16, (p - (75 - 2 n)) * 65536 + frac(m), E = 0 at the floor, and
 * nothing below the floor */
ACM_FEAT_HD static inline int32_t acm_feat_log_q16(uint64_t s_hi, uint64_t s_lo, uint32_t n, int32_t floor_q16)
{
	uint32_t m;
	const int p = acm_feat_lead(s_hi, s_lo, &m);
	if (p < 0)
		return floor_q16;
	const int32_t l = (p - (75 - 2 * (int)n)) * 65536 + (int32_t)acm_feat_log_frac(m);
	return l > floor_q16 ? l : floor_q16;
}

/* the output of include/acm_hip.h from L: V = ((L * mul + 2^23) >> 24) + offset, the shift arithmetic, as the bits of the float32
 * V * 2^-16 - exact, acm_feat_log_check keeps |V| below 2^24 */
ACM_FEAT_HD static inline uint32_t acm_feat_log_out(int32_t l, uint32_t mul_q24, int32_t offset_q16)
{
	const int64_t v = (((int64_t)l * (int64_t)mul_q24 + ((int64_t)1 << 23)) >> 24) + offset_q16;
	const float y = (float)(int32_t)v * (1.0f / 65536.0f);
	uint32_t bits;
	__builtin_memcpy(&bits, &y, sizeof bits);
	return bits;
}

/* what the feature kernel is launched over: items are (row, tile of ACM_FEAT_TILE frames), the grid is capped by the handle's
 * dense_grid like every dense kernel's, and a workgroup strides over the rest */
struct AcmFeatGeo {
	uint64_t frames;                /* F */
	uint64_t tiles;                 /* per row */
	uint64_t nwork;                 /* nrows * tiles */
	uint32_t grid;
	bool ok;                        /* false: more items than the kernel's counters are meant for */
};
static inline AcmFeatGeo acm_feat_geo(uint64_t nrows, uint64_t F, uint32_t dense_grid, uint32_t most)
{
	AcmFeatGeo g{};
	g.frames = F;
	g.tiles = (F + ACM_FEAT_TILE - 1) / ACM_FEAT_TILE;
	g.ok = g.tiles == 0 || nrows <= (1ull << 40) / g.tiles;
	g.nwork = g.ok ? nrows * g.tiles : 0;
	const uint32_t cap = acm_cap_value(dense_grid, most);
	g.grid = (uint32_t)(g.nwork < cap ? g.nwork : cap);
	return g;
}

/* column tiles of the DFT's B operand: bins [16 bt, 16 bt + 16) as a tile of cosines and a tile of sines, bins past N / 2 zero */
static inline uint32_t acm_feat_bin_tiles(uint32_t n_fft) { return n_fft / 32 + 1; }
/* bytes of the operand: per bin tile, part (cosine, sine), K step and byte plane (hi, lo) 64 lanes of 16 bytes */
static inline size_t acm_feat_twiddle_bytes(uint32_t n_fft) { return (size_t)acm_feat_bin_tiles(n_fft) * 2 * (n_fft / ACM_FEAT_KSTEP) * 2 * 1024; }

#ifdef __cplusplus
namespace acmbatch {

/* where the call's tables sit: the bank's, uploaded behind the filter pass's in the H_JOBS / D_JOBS arenas from a multiple of 64 on,
 * every table on a multiple of 16; and the feature arena: nrows rows of T int16 samples, slack, then the B operand on a multiple of 256 */
struct FeatLayout {
	acm_feat_bank bank{};
	uint32_t n = 0;                 /* log2 N */
	uint64_t T = 0, F = 0, nrows = 0;
	size_t n_weights = 0;           /* of mel_w that some band reaches */
	uint64_t out_words = 0;         /* nrows * B * F */
	size_t window_off() const { return 0; }
	size_t cs_off() const { return up16(window_off() + bank.n_fft * sizeof(int16_t)); }
	size_t first_off() const { return up16(cs_off() + bank.n_fft * sizeof(int16_t)); }
	size_t count_off() const { return up16(first_off() + bank.n_mels * sizeof(uint16_t)); }
	size_t off_off() const { return up16(count_off() + bank.n_mels * sizeof(uint16_t)); }
	size_t w_off() const { return up16(off_off() + bank.n_mels * sizeof(uint32_t)); }
	size_t table_bytes() const { return up16(w_off() + n_weights * sizeof(uint16_t)); }
	size_t rows_bytes() const { return (size_t)((nrows * T + ACM_FEAT_ROW_SLACK) * sizeof(int16_t)); }
	size_t twiddle_off() const { return (rows_bytes() + 255) / 256 * 256; }
	/* acm_batch_decode_windows_logmel: the scale (has_log), and with ACM_FEAT_LOG_TOP a table of the rows' maxima, nrows int32,
	 * behind the B operand on a multiple of 256 - a call without TOP has none, and its arena ends where a features call's does */
	bool has_log = false;
	acm_feat_log log{};
	bool top() const { return has_log && (log.flags & ACM_FEAT_LOG_TOP) != 0; }
	size_t rowmax_off() const { return (twiddle_off() + acm_feat_twiddle_bytes(bank.n_fft) + 255) / 256 * 256; }
	size_t rowmax_bytes() const { return top() ? (size_t)nrows * sizeof(int32_t) : 0; }
	size_t arena_bytes() const { return top() ? rowmax_off() + rowmax_bytes() : twiddle_off() + acm_feat_twiddle_bytes(bank.n_fft); }
	/* the tables as uploaded, into table_bytes() bytes at dst */
	void pack(uint8_t *dst) const;
	static size_t up16(size_t v) { return (v + 15) / 16 * 16; }
};

/* ACMHIP_OK, or ACMHIP_ERR_ARG for what include/acm_hip.h refuses of the bank, of channels or of the room behind d_pcm - then nothing
 * of `out` is to be used */
int acm_feat_prepare(const acm_feat_bank *bank, uint32_t channels, uint64_t T, uint64_t nrows, uint64_t d_pcm_words, FeatLayout *out);
/* ... and with `log` given, for what acm_batch_decode_windows_logmel refuses beyond that (acm_feat_log_check) */
int acm_feat_prepare(const acm_feat_bank *bank, const acm_feat_log *log, uint32_t channels, uint64_t T, uint64_t nrows, uint64_t d_pcm_words,
		     FeatLayout *out);

} // namespace acmbatch
#endif

#endif
