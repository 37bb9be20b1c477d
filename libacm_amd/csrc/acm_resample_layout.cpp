/*
 * acm_resample_layout.cpp - the ratios and the filters of ACM_DENSE_RESAMPLE and ACM_DENSE_SPEED (include/acm_hip.h), device-free: no
 * HIP call here.
 *
 * The filter is a Hann-windowed sinc of Z = 8 zero crossings a side, cut off at the lower of the two Nyquist rates.  Its exact form is
 * a polyphase table of L phases: designed in double, normalised per phase, rounded to Q14 (ties to even) and corrected on its largest
 * tap so that every phase sums to exactly 16384.  Its wide form, for a ratio whose L phases would not fit, is the same design at P + 1
 * equally spaced phases of a cutoff quantised to 64ths; the kernel interpolates between two neighbours.  Everything behind these
 * tables - the kernels, the tests' numpy models - is integer arithmetic.
 */
#include "acm_resample_layout.h"

#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <numeric>

#include "acm_hip.h"

namespace acmbatch {

bool acm_resample_ratio_lm(uint64_t L, uint64_t M, ResampleRatio *r)
{
	if (L == 0 || M == 0 || L > ACM_RESAMPLE_MAX_TAPS || M > ACM_RESAMPLE_MAX_DOWN * L)
		return false;
	const uint64_t Wd = L >= M ? ACM_RESAMPLE_ZEROS : (ACM_RESAMPLE_ZEROS * M + L - 1) / L;
	if (L * 2 * Wd > ACM_RESAMPLE_MAX_TAPS)
		return false;
	*r = ResampleRatio{ (uint32_t)L, (uint32_t)M, (uint32_t)(2 * Wd), (uint32_t)Wd };
	return true;
}

bool acm_resample_ratio(uint32_t rate_in, uint32_t rate_out, ResampleRatio *r)
{
	if (rate_in == 0 || rate_out == 0)
		return false;
	const uint32_t g = std::gcd(rate_in, rate_out);
	return acm_resample_ratio_lm(rate_out / g, rate_in / g, r);
}

void acm_wide_shape(uint32_t c, uint32_t *K, uint32_t *Wd, uint32_t *P, uint32_t *b)
{
	*Wd = c >= 64 ? ACM_RESAMPLE_ZEROS : (64 * ACM_RESAMPLE_ZEROS + c - 1) / c;
	*K = 2 * *Wd;
	*b = 0;
	while (((2u << *b) + 1) * *K <= ACM_RESAMPLE_MAX_TAPS)
		++*b;
	*P = 1u << *b;
}

SpeedFilter acm_speed_filter(uint32_t rate_in, uint32_t rate_out, uint32_t num, uint32_t den)
{
	SpeedFilter f;
	if (rate_in == 0 || rate_out == 0 || num == 0 || den == 0 || num > 0xFFFF || den > 0xFFFF)
		return f;
	const uint64_t up = (uint64_t)rate_out * den, down = (uint64_t)rate_in * num, g = std::gcd(up, down);
	const uint64_t L = up / g, M = down / g;
	if (L == M) {
		f.kind = SPEED_NONE;
		f.L = f.M = 1;
		f.K = 2 * ACM_RESAMPLE_ZEROS;
		f.Wd = ACM_RESAMPLE_ZEROS;
		return f;
	}
	if (M > ACM_RESAMPLE_MAX_DOWN * L)              /* (both below 2^48) */
		return f;
	ResampleRatio r;
	if (acm_resample_ratio_lm(L, M, &r)) {
		f.kind = SPEED_EXACT;
		f.L = r.L, f.M = r.M, f.K = r.K, f.Wd = r.Wd;
		return f;
	}
	if (L >= (1ull << 31) || M >= (1ull << 31))
		return f;
	f.kind = SPEED_WIDE;
	f.L = (uint32_t)L, f.M = (uint32_t)M;
	f.c = L >= M ? 64 : (uint32_t)(64 * L / M);
	acm_wide_shape(f.c, &f.K, &f.Wd, &f.P, &f.b);
	f.step = (M << 32) / L;
	return f;
}

/* one phase: the contract's h at the K offsets u[t] (source frames from the output's position), normalised, in Q14.  False where the
 * taps could overflow the kernels' 32-bit sums: no table inside the limits is known to */
static bool design_phase(const std::vector<double> &u, double s, int16_t *q)
{
	const double pi = 3.14159265358979323846, Z = ACM_RESAMPLE_ZEROS;
	const size_t K = u.size();
	std::vector<double> h(K);
	double sum = 0;
	for (size_t t = 0; t < K; t++) {
		const double v = u[t] * s / Z, x = s * u[t];
		const double sinc = x == 0 ? 1.0 : sin(pi * x) / (pi * x);
		h[t] = s * sinc * (fabs(v) < 1 ? 0.5 + 0.5 * cos(pi * v) : 0.0);
		sum += h[t];
	}
	long total = 0, mag = 0;
	size_t top = 0;
	for (size_t t = 0; t < K; t++) {
		const long v = lrint(nearbyint(h[t] / sum * 16384.0));          /* the default rounding mode: ties to even */
		q[t] = (int16_t)v;
		total += v;
		if (v > q[top])
			top = t;
	}
	q[top] = (int16_t)(q[top] + (16384 - total));
	for (size_t t = 0; t < K; t++)
		mag += labs((long)q[t]);
	return mag < 65536;
}

static std::shared_ptr<const ResampleTable> design(const ResampleRatio &r)
{
	auto tab = std::make_shared<ResampleTable>();
	tab->r = r;
	tab->q.resize((size_t)r.L * r.K);
	const double s = r.L >= r.M ? 1.0 : (double)r.L / (double)r.M;         /* the cutoff as a fraction of the source Nyquist */
	std::vector<double> u(r.K);
	for (uint32_t ph = 0; ph < r.L; ph++) {
		for (uint32_t t = 0; t < r.K; t++)
			u[t] = (((double)t - (double)r.Wd + 1.0) * (double)r.L - (double)ph) / (double)r.L;
		if (!design_phase(u, s, &tab->q[(size_t)ph * r.K]))
			return nullptr;
	}
	return tab;
}

static std::shared_ptr<const ResampleTable> design_wide(uint32_t c)
{
	auto tab = std::make_shared<ResampleTable>();
	tab->wide = true;
	tab->c = c;
	acm_wide_shape(c, &tab->r.K, &tab->r.Wd, &tab->P, &tab->b);
	tab->q.resize((size_t)(tab->P + 1) * tab->r.K);
	std::vector<double> u(tab->r.K);
	for (uint32_t p = 0; p <= tab->P; p++) {
		for (uint32_t t = 0; t < tab->r.K; t++)
			u[t] = ((double)t - (double)tab->r.Wd + 1.0) - (double)p / (double)tab->P;
		if (!design_phase(u, (double)c / 64.0, &tab->q[(size_t)p * tab->r.K]))
			return nullptr;
	}
	return tab;
}

/* exact tables by L << 32 | M, wide ones by c: the two do not meet, an exact table has L above 0 */
static std::shared_ptr<const ResampleTable> kept_table(uint64_t key, const ResampleRatio *r, uint32_t c)
{
	static std::mutex mu;
	static std::map<uint64_t, std::shared_ptr<const ResampleTable>> kept;
	{
		std::lock_guard<std::mutex> lock(mu);
		auto it = kept.find(key);
		if (it != kept.end())
			return it->second;
	}
	std::shared_ptr<const ResampleTable> tab = r ? design(*r) : design_wide(c);
	std::lock_guard<std::mutex> lock(mu);
	if (tab && kept.size() < 256)                   /* a corpus has a handful of ratios; beyond that a table is designed per call */
		kept.emplace(key, tab);
	return tab;
}

std::shared_ptr<const ResampleTable> acm_resample_table_lm(uint32_t L, uint32_t M)
{
	ResampleRatio r;
	if (!acm_resample_ratio_lm(L, M, &r))
		return nullptr;
	return kept_table((uint64_t)L << 32 | M, &r, 0);
}

std::shared_ptr<const ResampleTable> acm_resample_table(uint32_t rate_in, uint32_t rate_out)
{
	ResampleRatio r;
	if (!acm_resample_ratio(rate_in, rate_out, &r))
		return nullptr;
	return acm_resample_table_lm(r.L, r.M);
}

std::shared_ptr<const ResampleTable> acm_wide_table(uint32_t c)
{
	if (c < 64 / ACM_RESAMPLE_MAX_DOWN || c > 64)
		return nullptr;
	return kept_table(c, nullptr, c);
}

std::shared_ptr<const ResampleTable> acm_speed_table(const SpeedFilter &f)
{
	return f.kind == SPEED_EXACT ? acm_resample_table_lm(f.L, f.M) : f.kind == SPEED_WIDE ? acm_wide_table(f.c) : nullptr;
}

} // namespace acmbatch

extern "C" uint64_t acm_dense_resampled_frames(uint64_t source_frames, uint32_t rate_in, uint32_t rate_out)
{
	acmbatch::ResampleRatio r;
	if (!acmbatch::acm_resample_ratio(rate_in, rate_out, &r) || source_frames > (1ull << 50))
		return UINT64_MAX;
	return rate_in == rate_out ? source_frames : acmbatch::acm_resample_frames(source_frames, r);
}

extern "C" int acm_dense_resample_taps(uint32_t rate_in, uint32_t rate_out, uint32_t *L, uint32_t *M, uint32_t *K, uint32_t *Wd, int16_t *taps,
				       size_t cap)
{
	acmbatch::ResampleRatio r;
	if (!acmbatch::acm_resample_ratio(rate_in, rate_out, &r))
		return ACMHIP_ERR_ARG;
	if (L)
		*L = r.L;
	if (M)
		*M = r.M;
	if (K)
		*K = r.K;
	if (Wd)
		*Wd = r.Wd;
	if (!taps)
		return ACMHIP_OK;
	const std::shared_ptr<const acmbatch::ResampleTable> tab = acmbatch::acm_resample_table(rate_in, rate_out);
	if (!tab || cap < tab->q.size())
		return ACMHIP_ERR_ARG;
	std::copy(tab->q.begin(), tab->q.end(), taps);
	return ACMHIP_OK;
}

extern "C" uint64_t acm_dense_speed_frames(uint64_t source_frames, uint32_t rate_in, uint32_t rate_out, uint32_t num, uint32_t den)
{
	const acmbatch::SpeedFilter f = acmbatch::acm_speed_filter(rate_in, rate_out, num, den);
	if (f.kind == acmbatch::SPEED_BAD || source_frames > (1ull << 50))
		return UINT64_MAX;
	return f.kind == acmbatch::SPEED_NONE ? source_frames : acmbatch::acm_resample_frames(source_frames, f.L, f.M);
}

extern "C" int acm_dense_speed_taps(uint32_t rate_in, uint32_t rate_out, uint32_t num, uint32_t den, acm_dense_speed_info *info, int16_t *taps,
				    size_t cap)
{
	using namespace acmbatch;
	SpeedFilter f = acm_speed_filter(rate_in, rate_out, num, den);
	if (f.kind == SPEED_BAD)
		return ACMHIP_ERR_ARG;
	if (info)
		*info = acm_dense_speed_info{ (uint32_t)f.kind, f.L, f.M, f.K, f.Wd, f.P, f.c, f.kind == SPEED_WIDE ? f.P + 1 : f.L, f.step };
	if (!taps)
		return ACMHIP_OK;
	if (f.kind == SPEED_NONE)
		f.kind = SPEED_EXACT;                   /* the identity: one tap of 16384 */
	const std::shared_ptr<const ResampleTable> tab = acm_speed_table(f);
	if (!tab || cap < tab->q.size())
		return ACMHIP_ERR_ARG;
	std::copy(tab->q.begin(), tab->q.end(), taps);
	return ACMHIP_OK;
}
