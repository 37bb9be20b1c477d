/*
 * acm_resample_layout.h - ACM_DENSE_RESAMPLE of acm_batch_decode_windows_dense (include/acm_hip.h) without a device: which ratio of
 * sample rates the dense writer takes, how many frames a resampled row has, and the Q14 filter a ratio has - designed here, once, in
 * double; what the kernel (acm_dense_resample.hip) reads is this table uploaded.  Internal; acm_dense_layout.cpp is the user.
 */
#ifndef ACM_RESAMPLE_LAYOUT_H
#define ACM_RESAMPLE_LAYOUT_H

#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <vector>

namespace acmbatch {

constexpr uint32_t ACM_RESAMPLE_ZEROS = 8;              /* Z: zero crossings of the sinc on either side */
constexpr uint32_t ACM_RESAMPLE_MAX_DOWN = 8;           /* M <= 8 * L */
constexpr uint32_t ACM_RESAMPLE_MAX_TAPS = 16384;       /* L * K: a table of 32 KB, what the kernel keeps in LDS */
constexpr size_t ACM_RESAMPLE_MAX_RATIOS = 16;          /* distinct ratios of one call */

struct ResampleRatio {
	uint32_t L = 0, M = 0, K = 0, Wd = 0;           /* rate_out / g, rate_in / g, taps per phase, taps from the centre back */
};

/* whether rate_in -> rate_out is a ratio the dense writer takes, and then its numbers.  rate_in == rate_out: L = M = 1 and, of the 16 taps, one that is 16384 */
bool acm_resample_ratio(uint32_t rate_in, uint32_t rate_out, ResampleRatio *r);

/* ceil(f * L / M): the frames of a row resampled from f source frames (f below 2^50) */
inline uint64_t acm_resample_frames(uint64_t f, const ResampleRatio &r) { return (f * r.L + r.M - 1) / r.M; }

struct ResampleTable {
	uint32_t rate_in = 0, rate_out = 0;
	ResampleRatio r;
	std::vector<int16_t> q;                         /* [L][K], every phase sums to 16384 */
};

/* the table of a supported ratio; null for an unsupported one.  Tables are designed once a process and kept */
std::shared_ptr<const ResampleTable> acm_resample_table(uint32_t rate_in, uint32_t rate_out);

} // namespace acmbatch

#endif
