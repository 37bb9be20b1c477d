/*
 * acm_feat_layout.cpp - the device-free half of acm_batch_decode_windows_features (acm_batch_windows.cpp): the bank's validation
 * (acm_feat_bank_check, the one text of it), the frame count, the designed tables and the call's layout.  No HIP call here.
 */
#include "acm_feat_layout.h"

#include <math.h>
#include <string.h>

#include <vector>

static uint32_t log2_fft(uint32_t n_fft)
{
	for (uint32_t n = 7; n <= 11; n++)
		if (n_fft == 1u << n)
			return n;
	return 0;
}

extern "C" int acm_feat_bank_check(const acm_feat_bank *b)
{
	if (!b || !log2_fft(b->n_fft) || b->hop == 0 || b->hop > b->n_fft || b->n_mels == 0 || b->n_mels > ACM_FEAT_MAX_MELS ||
	    (b->flags & ~(ACM_FEAT_CENTER | ACM_FEAT_TIME_MAJOR)) != 0 || b->reserved != 0)
		return ACMHIP_ERR_ARG;
	if (!b->window || !b->cs || !b->mel_first || !b->mel_count || !b->mel_off || !b->mel_w)
		return ACMHIP_ERR_ARG;
	for (uint32_t t = 0; t < b->n_fft; t++)
		if (b->window[t] < 0 || b->window[t] > ACM_FEAT_WINDOW_MAX || b->cs[t] < -ACM_FEAT_CS_ONE || b->cs[t] > ACM_FEAT_CS_ONE)
			return ACMHIP_ERR_ARG;
	for (uint32_t m = 0; m < b->n_mels; m++) {
		if ((uint32_t)b->mel_first[m] + b->mel_count[m] > b->n_fft / 2 + 1)
			return ACMHIP_ERR_ARG;
		for (uint32_t i = 0; i < b->mel_count[m]; i++)
			if (b->mel_w[(size_t)b->mel_off[m] + i] > ACM_FEAT_W_ONE)
				return ACMHIP_ERR_ARG;
	}
	return ACMHIP_OK;
}

extern "C" int acm_feat_log_check(const acm_feat_bank *b, const acm_feat_log *g)
{
	if (acm_feat_bank_check(b) != ACMHIP_OK || !g || (g->flags & ~ACM_FEAT_LOG_TOP) != 0 || g->reserved != 0)
		return ACMHIP_ERR_ARG;
	if (g->floor_q16 < -ACM_FEAT_LOG_FLOOR_MAX || g->floor_q16 > ACM_FEAT_LOG_FLOOR_MAX || g->mul_q24 == 0 || g->mul_q24 > ACM_FEAT_LOG_MUL_MAX ||
	    g->top_q16 > ACM_FEAT_LOG_TOP_MAX || (g->top_q16 != 0 && !(g->flags & ACM_FEAT_LOG_TOP)))
		return ACMHIP_ERR_ARG;
	/* |V| stays below 2^24: |L| <= Lb, the largest |log2 y| of any bank (p in [0, 88], n in [7, 11]) or the floor */
	const int64_t fl = g->floor_q16 < 0 ? -(int64_t)g->floor_q16 : g->floor_q16, off = g->offset_q16 < 0 ? -(int64_t)g->offset_q16 : g->offset_q16;
	const int64_t lb = fl > 62 * 65536 ? fl : 62 * 65536;
	return ((lb * (int64_t)g->mul_q24) >> 24) + off + 1 < ((int64_t)1 << 24) ? ACMHIP_OK : ACMHIP_ERR_ARG;
}

extern "C" uint64_t acm_feat_frames(uint64_t T, const acm_feat_bank *b)
{
	if (!b || b->hop == 0)
		return 0;
	if (b->flags & ACM_FEAT_CENTER)
		return 1 + T / b->hop;
	return T >= b->n_fft ? 1 + (T - b->n_fft) / b->hop : 0;
}

static double hz_to_mel(double f) { return 2595.0 * log10(1.0 + f / 700.0); }
static double mel_to_hz(double m) { return 700.0 * (pow(10.0, m / 2595.0) - 1.0); }

extern "C" int acm_feat_design(uint32_t rate, uint32_t n_fft, uint32_t win_length, uint32_t hop, uint32_t n_mels, double f_min, double f_max,
			       uint32_t flags, int16_t *window, int16_t *cs, uint16_t *mel_first, uint16_t *mel_count, uint32_t *mel_off, uint16_t *mel_w,
			       size_t weights_cap, size_t *n_weights)
{
	if (n_weights)
		*n_weights = 0;
	if (rate == 0 || !log2_fft(n_fft) || win_length == 0 || win_length > n_fft || hop == 0 || hop > n_fft || n_mels == 0 ||
	    n_mels > ACM_FEAT_MAX_MELS || (flags & ~(ACM_FEAT_CENTER | ACM_FEAT_TIME_MAJOR)) != 0 || !(f_min >= 0.0) || !(f_max > f_min) ||
	    !(f_max <= rate / 2.0))
		return ACMHIP_ERR_ARG;
	const double two_pi = 6.283185307179586476925286766559;
	if (window) {
		const uint32_t at = (n_fft - win_length) / 2;
		memset(window, 0, n_fft * sizeof(int16_t));
		for (uint32_t i = 0; i < win_length; i++)
			window[at + i] = (int16_t)nearbyint(ACM_FEAT_WINDOW_MAX * (0.5 - 0.5 * cos(two_pi * i / win_length)));
	}
	if (cs)
		for (uint32_t m = 0; m < n_fft; m++)
			cs[m] = (int16_t)nearbyint(ACM_FEAT_CS_ONE * cos(two_pi * m / n_fft));
	/* the B + 2 corner frequencies, equally spaced in mel; band b rises from corner b to corner b + 1 and falls to corner b + 2 */
	const double m_lo = hz_to_mel(f_min), m_hi = hz_to_mel(f_max);
	std::vector<double> corner(n_mels + 2);
	for (uint32_t i = 0; i < n_mels + 2; i++)
		corner[i] = mel_to_hz(m_lo + (m_hi - m_lo) * i / (n_mels + 1));
	const uint32_t bins = n_fft / 2 + 1;
	std::vector<uint16_t> q(bins);
	size_t total = 0;
	for (uint32_t b = 0; b < n_mels; b++) {
		uint32_t first = 0, last = 0;
		bool any = false;
		for (uint32_t k = 0; k < bins; k++) {
			const double f = (double)k * rate / n_fft;
			const double up = (f - corner[b]) / (corner[b + 1] - corner[b]), down = (corner[b + 2] - f) / (corner[b + 2] - corner[b + 1]);
			const double w = fmax(0.0, fmin(up, down));
			q[k] = (uint16_t)nearbyint(ACM_FEAT_W_ONE * w);
			if (q[k]) {
				if (!any)
					first = k;
				last = k;
				any = true;
			}
		}
		const uint32_t count = any ? last - first + 1 : 0;
		if (mel_first)
			mel_first[b] = (uint16_t)first;
		if (mel_count)
			mel_count[b] = (uint16_t)count;
		if (mel_off)
			mel_off[b] = (uint32_t)total;
		if (mel_w) {
			if (total + count > weights_cap)
				return ACMHIP_ERR_ARG;
			memcpy(mel_w + total, q.data() + first, count * sizeof(uint16_t));
		}
		total += count;
		if (n_weights)
			*n_weights = total;
	}
	return ACMHIP_OK;
}

namespace acmbatch {

int acm_feat_prepare(const acm_feat_bank *bank, uint32_t channels, uint64_t T, uint64_t nrows, uint64_t d_pcm_words, FeatLayout *out)
{
	FeatLayout &L = *out;
	L = FeatLayout();
	if (channels != 1 || acm_feat_bank_check(bank) != ACMHIP_OK)
		return ACMHIP_ERR_ARG;
	L.bank = *bank;
	L.n = log2_fft(bank->n_fft);
	L.T = T;
	L.nrows = nrows;
	L.F = acm_feat_frames(T, bank);
	for (uint32_t m = 0; m < bank->n_mels; m++)
		if (bank->mel_count[m] && (size_t)bank->mel_off[m] + bank->mel_count[m] > L.n_weights)
			L.n_weights = (size_t)bank->mel_off[m] + bank->mel_count[m];
	const uint64_t per_row = L.F * bank->n_mels;
	if (per_row && nrows > ~0ull / per_row)
		return ACMHIP_ERR_ARG;
	L.out_words = nrows * per_row;
	return d_pcm_words >= L.out_words ? ACMHIP_OK : ACMHIP_ERR_ARG;
}

int acm_feat_prepare(const acm_feat_bank *bank, const acm_feat_log *log, uint32_t channels, uint64_t T, uint64_t nrows, uint64_t d_pcm_words,
		     FeatLayout *out)
{
	if (acm_feat_prepare(bank, channels, T, nrows, d_pcm_words, out) != ACMHIP_OK || acm_feat_log_check(bank, log) != ACMHIP_OK)
		return ACMHIP_ERR_ARG;
	out->has_log = true;
	out->log = *log;
	return ACMHIP_OK;
}

void FeatLayout::pack(uint8_t *dst) const
{
	memset(dst, 0, table_bytes());
	memcpy(dst + window_off(), bank.window, bank.n_fft * sizeof(int16_t));
	memcpy(dst + cs_off(), bank.cs, bank.n_fft * sizeof(int16_t));
	memcpy(dst + first_off(), bank.mel_first, bank.n_mels * sizeof(uint16_t));
	memcpy(dst + count_off(), bank.mel_count, bank.n_mels * sizeof(uint16_t));
	memcpy(dst + off_off(), bank.mel_off, bank.n_mels * sizeof(uint32_t));
	if (n_weights)
		memcpy(dst + w_off(), bank.mel_w, n_weights * sizeof(uint16_t));
}

} // namespace acmbatch
