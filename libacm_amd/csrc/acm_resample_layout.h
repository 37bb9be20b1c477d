/*
 * acm_resample_layout.h - ACM_DENSE_RESAMPLE and ACM_DENSE_SPEED of acm_batch_decode_windows_dense (include/acm_hip.h) without a
 * device: which ratio of sample rates, times a window's speed, the dense writer takes and in which of its two filter forms, how many
 * frames a resampled row has, and the Q14 table of a ratio or a cutoff - designed here, once, in double; what the kernels
 * (acm_dense_resample.hip, acm_dense_speed.hip) read is this table uploaded.  Internal; acm_dense_layout.cpp is the user.
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

/* whether rate_in -> rate_out is a ratio the exact filter takes, and then its numbers.  rate_in == rate_out: L = M = 1 and, of the 16 taps, one that is 16384 */
bool acm_resample_ratio(uint32_t rate_in, uint32_t rate_out, ResampleRatio *r);
/* the same from the ratio itself: L / M in lowest terms, both above 0 */
bool acm_resample_ratio_lm(uint64_t L, uint64_t M, ResampleRatio *r);

/* ceil(f * L / M): the frames of a row resampled from f source frames, whatever f (L, M below 2^32); all ones where 64 bits do not hold it */
inline uint64_t acm_resample_frames(uint64_t f, uint64_t L, uint64_t M)
{
	const unsigned __int128 n = ((unsigned __int128)f * L + M - 1) / M;
	return n > (unsigned __int128)UINT64_MAX ? UINT64_MAX : (uint64_t)n;
}
inline uint64_t acm_resample_frames(uint64_t f, const ResampleRatio &r) { return acm_resample_frames(f, r.L, r.M); }

/* ACM_DENSE_SPEED: what a window of a file at rate_in, played at num / den, gets in a batch at rate_out.  L = rate_out * den / g,
 * M = rate_in * num / g.  NONE: L == M, the row is not filtered.  EXACT: the polyphase table of (L, M), K and Wd its.  WIDE: the
 * interpolated table of cutoff c (64ths of the source Nyquist), P = 2^b prototype phases and one more, K and Wd that table's, step =
 * floor(M * 2^32 / L).  BAD: turned away - no rate, no speed, M > 8 L, or L or M of 2^31 and more where the exact table is too large */
enum SpeedKind { SPEED_BAD = -1, SPEED_NONE = 0, SPEED_EXACT = 1, SPEED_WIDE = 2 };
struct SpeedFilter {
	int kind = SPEED_BAD;
	uint32_t L = 0, M = 0, K = 0, Wd = 0;
	uint32_t c = 0, P = 0, b = 0;                   /* WIDE alone */
	uint64_t step = 0;
};
SpeedFilter acm_speed_filter(uint32_t rate_in, uint32_t rate_out, uint32_t num, uint32_t den);

/* a table the kernels read: the exact one of a ratio (wide == false; r is the ratio's; L phases) or the wide one of a cutoff (c, P, b;
 * r.K and r.Wd its taps, r.L = r.M = 0; P + 1 phases) */
struct ResampleTable {
	ResampleRatio r;
	bool wide = false;
	uint32_t c = 0, P = 0, b = 0;
	std::vector<int16_t> q;                         /* [phases][K], every phase sums to 16384 */
	uint32_t phases() const { return wide ? P + 1 : r.L; }
};

/* K, Wd, P and b of the wide table of cutoff c (8 .. 64) */
void acm_wide_shape(uint32_t c, uint32_t *K, uint32_t *Wd, uint32_t *P, uint32_t *b);

/* the table of a supported ratio; null for an unsupported one.  Tables are a function of (L, M), designed once a process and kept */
std::shared_ptr<const ResampleTable> acm_resample_table(uint32_t rate_in, uint32_t rate_out);
std::shared_ptr<const ResampleTable> acm_resample_table_lm(uint32_t L, uint32_t M);
/* ... and the wide one of a cutoff, a function of c alone: 57 at most */
std::shared_ptr<const ResampleTable> acm_wide_table(uint32_t c);
/* the table a filter reads; null for NONE and BAD */
std::shared_ptr<const ResampleTable> acm_speed_table(const SpeedFilter &f);

} // namespace acmbatch

#endif
