/*
 * acm_resample_layout.cpp - the ratios and the filter of ACM_DENSE_RESAMPLE (include/acm_hip.h), device-free: no HIP call here.
 *
 * The filter is a Hann-windowed sinc of Z = 8 zero crossings a side, cut off at the lower of the two Nyquist rates, as a polyphase
 * table of L phases: designed in double, normalised per phase, rounded to Q14 (ties to even) and corrected on its largest tap so that
 * every phase sums to exactly 16384.  Everything behind this table - the kernel, the tests' numpy model - is integer arithmetic.
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

bool acm_resample_ratio(uint32_t rate_in, uint32_t rate_out, ResampleRatio *r)
{
	if (rate_in == 0 || rate_out == 0)
		return false;
	const uint32_t g = std::gcd(rate_in, rate_out);
	const uint64_t L = rate_out / g, M = rate_in / g;
	if (M > ACM_RESAMPLE_MAX_DOWN * L)
		return false;
	const uint64_t Wd = L >= M ? ACM_RESAMPLE_ZEROS : (ACM_RESAMPLE_ZEROS * M + L - 1) / L;
	if (L * 2 * Wd > ACM_RESAMPLE_MAX_TAPS)
		return false;
	*r = ResampleRatio{ (uint32_t)L, (uint32_t)M, (uint32_t)(2 * Wd), (uint32_t)Wd };
	return true;
}

/* null where a phase's taps could overflow the kernel's 32-bit sum: no ratio inside the limits is known to */
static std::shared_ptr<const ResampleTable> design(uint32_t rate_in, uint32_t rate_out, const ResampleRatio &r)
{
	auto tab = std::make_shared<ResampleTable>();
	tab->rate_in = rate_in;
	tab->rate_out = rate_out;
	tab->r = r;
	tab->q.resize((size_t)r.L * r.K);
	const double pi = 3.14159265358979323846, Z = ACM_RESAMPLE_ZEROS;
	const double s = r.L >= r.M ? 1.0 : (double)r.L / (double)r.M;         /* the cutoff as a fraction of the source Nyquist */
	std::vector<double> h(r.K);
	for (uint32_t ph = 0; ph < r.L; ph++) {
		double sum = 0;
		for (uint32_t t = 0; t < r.K; t++) {
			const double a = ((double)t - (double)r.Wd + 1.0) * (double)r.L - (double)ph;
			const double u = a / (double)r.L, v = u * s / Z, x = s * u;
			const double sinc = x == 0 ? 1.0 : sin(pi * x) / (pi * x);
			h[t] = s * sinc * (fabs(v) < 1 ? 0.5 + 0.5 * cos(pi * v) : 0.0);
			sum += h[t];
		}
		int16_t *q = &tab->q[(size_t)ph * r.K];
		long total = 0, mag = 0;
		uint32_t top = 0;
		for (uint32_t t = 0; t < r.K; t++) {
			const long v = lrint(nearbyint(h[t] / sum * 16384.0));          /* the default rounding mode: ties to even */
			q[t] = (int16_t)v;
			total += v;
			if (v > q[top])
				top = t;
		}
		q[top] = (int16_t)(q[top] + (16384 - total));
		for (uint32_t t = 0; t < r.K; t++)
			mag += labs((long)q[t]);
		if (mag >= 65536)
			return nullptr;
	}
	return tab;
}

std::shared_ptr<const ResampleTable> acm_resample_table(uint32_t rate_in, uint32_t rate_out)
{
	ResampleRatio r;
	if (!acm_resample_ratio(rate_in, rate_out, &r))
		return nullptr;
	static std::mutex mu;
	static std::map<uint64_t, std::shared_ptr<const ResampleTable>> kept;
	const uint64_t key = (uint64_t)rate_in << 32 | rate_out;
	{
		std::lock_guard<std::mutex> lock(mu);
		auto it = kept.find(key);
		if (it != kept.end())
			return it->second;
	}
	std::shared_ptr<const ResampleTable> tab = design(rate_in, rate_out, r);
	std::lock_guard<std::mutex> lock(mu);
	if (tab && kept.size() < 256)                   /* a corpus has a handful of rates; beyond that a table is designed per call */
		kept.emplace(key, tab);
	return tab;
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
