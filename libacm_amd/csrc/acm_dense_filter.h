/*
 * acm_dense_filter.h - what acm_dense_resample.hip and acm_dense_speed.hip share: one unit of one sub-row of a dense crop batch for
 * a row that is filtered - by the exact polyphase table of ACM_DENSE_RESAMPLE or, WIDE, by the interpolated table of ACM_DENSE_SPEED
 * (include/acm_hip.h); a row that is not filtered takes acm_dense_gather.h's gather.  Device code, in an unnamed namespace of the
 * including file.
 *
 * The exact filter, on integers: for output frame j of a channel,
 *   n = j * M;  base = n / L;  ph = n % L;  acc = sum over t < K of q[ph][t] * x[base - Wd + 1 + t];  y = clamp((acc + 8192) >> 14)
 * with x the row's source frames AFTER their channel conversion, zero outside [0, frames_in), and q the ratio's Q14 table.  The wide
 * one: X = j * step; base = X >> 32; p and w from X's fraction; the sums a0 over q[p] and a1 over q[p + 1];
 * y = clamp((a0 + (((a1 - a0) * w) >> 15) + 8192) >> 14).  32-bit sums: a phase's |q| add up to less than 65536.
 *
 * A filtered unit
 *   1. copies the row's table - 32 KB at most - into LDS: the lanes' phases differ, so the taps are gathered;
 *   2. stages the source span of its outputs, converted, as one plane per output channel of the sub-row in LDS, zeros where the span
 *      reaches in front of the row's first frame or behind its last: lanes load the aligned 16-byte lines that hold a sample of the
 *      span - so every load lies inside the row's own samples rounded out to 16 bytes, which a window's 64-sample slot contains -
 *      and de-interleave, down-mix or duplicate on the way into LDS;
 *   3. has every lane filter its 8 consecutive outputs from LDS - base and phase by one division (WIDE: one 64-bit multiply) a lane,
 *      then by stepping - and store them as whole 16-byte lines where the output is aligned; the up to 7 samples in front of a row's
 *      first line and behind its last one are single outputs with narrow stores, as in acm_dense_gather.h.
 *
 * Table and planes share 63 KB of LDS, so two workgroups fit a CU's 160 KB.  The planes hold SPAN_CAP samples; a unit whose span is
 * longer (M / L above about 7.5: two planes hold half the frames each) is worked off in 2, 4, ... passes of 1024, 512, ... outputs,
 * each staging its own span.  No scratch: every register array is indexed by constants after unrolling.  No float arithmetic before
 * the final times 2^-15.
 */
#ifndef ACM_DENSE_FILTER_H
#define ACM_DENSE_FILTER_H

#include "acm_dense_gather.h"

namespace {

constexpr uint32_t TAB_CAP = 16384;             /* int16 of a ratio's table: ACM_RESAMPLE_MAX_TAPS */
constexpr uint32_t SPAN_CAP = 15872;            /* int16 of the staged planes: with the table 63 KB */

/* K products from the table and a plane, rounded and saturated */
__device__ __forceinline__ int filter_one(const int16_t *tab, const int16_t *x, uint32_t K)
{
	int acc = 0;
	for (uint32_t t = 0; t < K; t++)
		acc += (int)tab[t] * (int)x[t];
	return min(max((acc + 8192) >> 14, -32768), 32767);
}

/* the wide filter's last lines: between the sums of two neighbouring phases by w / 32768, in 64 bits, then rounded and saturated */
__device__ __forceinline__ int blend(int a0, int a1, uint32_t w)
{
	const int64_t acc = (int64_t)a0 + ((((int64_t)a1 - (int64_t)a0) * (int64_t)w) >> 15);
	return (int)min(max((acc + 8192) >> 14, (int64_t)-32768), (int64_t)32767);
}

/* ... of one output: phase p begins at tab, phase p + 1 lies K taps behind it */
__device__ __forceinline__ int filter_wide_one(const int16_t *tab, const int16_t *x, uint32_t K, uint32_t w)
{
	int a0 = 0, a1 = 0;
	for (uint32_t t = 0; t < K; t++) {
		a0 += (int)tab[t] * (int)x[t];
		a1 += (int)tab[K + t] * (int)x[t];
	}
	return blend(a0, a1, w);
}

/* One unit of one sub-row of a filtered row.  from: the row's source samples, r.frames_in frames of one or two samples - the other
 * count than the batch's where the row converts; plane: which channel a PLANAR sub-row is.  tab, xs: the table and the planes in LDS.
 * WIDE (ROW = AcmSpeedRow): the row takes the wide filter of ACM_DENSE_SPEED - a frame's position is its number times r.step in 32.32
 * fixed point, its phase the top r.b bits of the fraction, its weight the 15 bits behind them, and every tap feeds two sums */
template <typename OUT, int LAYOUT, bool WIDE, typename ROW>
__device__ __forceinline__ void filtered_sub_row(const int16_t *from, bool converts, uint32_t plane, const ROW &r, const int16_t *taps,
						 OUT *o, uint64_t sub_len, uint32_t unit, uint32_t units, int16_t *tab, int16_t *xs)
{
	constexpr uint32_t EPF = LAYOUT == INTER ? 2 : 1;              /* elements of the sub-row per frame = planes staged */
	const uint32_t src_c = LAYOUT == MONO ? (converts ? 2 : 1) : (converts ? 1 : 2);
	const uint32_t L = r.L, M = r.M, Wd = r.Wd, K = 2 * Wd, tid = threadIdx.x;
	const uint32_t qM = M / L, rM = M - qM * L;                     /* a frame's step: base += qM, ph += rM, with a carry */
	const int64_t f_in = (int64_t)r.frames_in;
	uint64_t step = 0;
	uint32_t b = 0;
	if constexpr (WIDE) {
		step = r.step;
		b = r.b;
	}
	/* the source frame output frame j is centred on */
	auto base_of = [&](uint64_t j) { return WIDE ? (j * step) >> 32 : j * M / L; };

	/* 1. the table, dword by dword: K is even and a table begins on a 16-byte line */
	{
		const uint32_t *g = reinterpret_cast<const uint32_t *>(taps + r.tab);
		uint32_t *l = reinterpret_cast<uint32_t *>(tab);
		const uint32_t phases = WIDE ? (1u << b) + 1 : L;
		for (uint32_t i = tid; i < phases * K / 2; i += DENSE_BLOCK)
			l[i] = g[i];
	}

	/* the sub-row as every gather cuts it: [0, head) in front of the first aligned output line, whole vectors, [tail, sub_len) */
	const SubCut c = cut_sub_row(o, sub_len);
	const uint64_t head = c.head, tail = c.tail;
	const uint64_t n_el = min(sub_len, r.n_out * EPF);              /* elements behind these are zero */
	const uint64_t bs = head + (uint64_t)unit * DENSE_UNIT, be = min(bs + DENSE_UNIT, tail);       /* the unit's vectors: elements [bs, be) */

	/* outputs a pass: as many as keep the planes inside SPAN_CAP, the up to 7 + 7 single outputs of a row's ends included.  n frames
	 * are centred on at most ceil(n * M / L) source frames - by the fixed-point bases, floor(n * step / 2^32) + 1 */
	uint32_t P = DENSE_UNIT;
	auto reach = [&](uint64_t n) { return WIDE ? ((n * step) >> 32) + 1 : (n * M + L - 1) / L; };
	while (EPF * (reach((uint64_t)(P + 16) / EPF) + K + 2) > SPAN_CAP)
		P >>= 1;
	const uint32_t plane_len = SPAN_CAP / EPF;

	/* the aligned line the row's first sample lies in, and how many samples into it */
	const uint32_t o_src = ((uint32_t)reinterpret_cast<uintptr_t>(from) & 15u) / 2;
	const u32x4 *lines = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(from) - 2 * o_src);

	for (uint64_t plo = bs;; plo += P) {
		const uint64_t phi = min(plo + P, be);
		const bool last = plo + P >= be;                        /* of the unit's passes */
		/* elements this pass writes: its vectors, and the ends of the row where it holds them */
		const uint64_t elo = unit == 0 && plo == bs ? 0 : plo;
		const uint64_t ehi = last && unit == units - 1 ? sub_len : phi;
		const uint64_t chi = min(ehi, n_el);                    /* ... of which [elo, chi) are computed */
		int64_t s0 = 0;
		if (chi > elo) {
			/* 2. the span: source frames [s0, s0 + span) serve the output frames [jlo, jhi) */
			const uint64_t jlo = elo / EPF, jhi = (chi + EPF - 1) / EPF;
			const uint64_t base_lo = base_of(jlo), base_hi = base_of(jhi - 1);
			s0 = (int64_t)base_lo - (int64_t)Wd + 1;
			const uint32_t span = (uint32_t)(base_hi - base_lo) + K;
			const int64_t fa = max(s0, (int64_t)0), fb = min(s0 + (int64_t)span, f_in);
			for (uint32_t i = tid; i < span; i += DENSE_BLOCK) {
				const int64_t fr = s0 + i;
				if (fr < fa || fr >= fb) {
					xs[i] = 0;
					if (EPF == 2)
						xs[plane_len + i] = 0;
				}
			}
			if (fb > fa) {
				const int64_t sa = fa * src_c, sb = fb * src_c;         /* samples of the row */
				const uint64_t l0 = (uint64_t)(o_src + sa) / 8, l1 = (uint64_t)(o_src + sb + 7) / 8;
				for (uint64_t li = l0 + tid; li < l1; li += DENSE_BLOCK) {
					const u32x4 v = lines[li];
					const uint32_t d[4] = { v.x, v.y, v.z, v.w };
					const int64_t s_line = (int64_t)(8 * li) - o_src;       /* the row's sample the line begins with */
					if (src_c == 1) {
#pragma unroll
						for (int p = 0; p < 8; p++) {
							const int64_t s = s_line + p;
							if (s >= sa && s < sb) {
								const int16_t val = (int16_t)(p & 1 ? d[p / 2] >> 16 : d[p / 2] & 0xFFFFu);
								xs[s - s0] = val;
								if (EPF == 2)
									xs[plane_len + (s - s0)] = val;
							}
						}
					} else {
						/* a stereo row begins on a dword: a dword is a frame */
#pragma unroll
						for (int p = 0; p < 4; p++) {
							const int64_t s = s_line + 2 * p;
							if (s >= sa && s < sb) {
								const int lft = (int16_t)(d[p] & 0xFFFFu), rgt = (int16_t)(d[p] >> 16);
								const int64_t at = s / 2 - s0;
								if (LAYOUT == MONO) {
									xs[at] = (int16_t)((lft + rgt) >> 1);
								} else if (LAYOUT == INTER) {
									xs[at] = (int16_t)lft;
									xs[plane_len + at] = (int16_t)rgt;
								} else {
									xs[at] = (int16_t)(plane ? rgt : lft);
								}
							}
						}
					}
				}
			}
		}
		__syncthreads();

		/* 3. the pass's vectors: lane tid writes elements [e0, e0 + 8) */
		const uint64_t e0 = plo + (uint64_t)tid * DENSE_VEC;
		if (e0 < phi) {
			int y[DENSE_VEC];
			if (e0 < chi) {
				/* the frames of the vector: 8, or with two elements a frame the 5 that 8 elements from an odd one on touch */
				constexpr int NF = EPF == 2 ? 5 : DENSE_VEC;
				const uint64_t j0 = e0 / EPF;
				/* where a frame's taps and source begin: ph * K into the table, base - Wd + 1 - s0 into a plane */
				uint32_t ftap[NF], foff[NF], fw[NF];
				if constexpr (WIDE) {
					/* one 64-bit multiply for the first frame, then the step */
					uint64_t X = j0 * step;
#pragma unroll
					for (int m = 0; m < NF; m++) {
						const uint32_t frac = (uint32_t)X;
						ftap[m] = (frac >> (32 - b)) * K;
						fw[m] = (frac >> (17 - b)) & 32767u;
						foff[m] = (uint32_t)((int64_t)(X >> 32) - (int64_t)Wd + 1 - s0);
						X += step;
					}
				} else {
					const uint64_t n0 = j0 * M;
					uint64_t base = n0 / L;
					uint32_t ph = (uint32_t)(n0 - base * L);
#pragma unroll
					for (int m = 0; m < NF; m++) {
						ftap[m] = ph * K;
						foff[m] = (uint32_t)((int64_t)base - (int64_t)Wd + 1 - s0);
						base += qM;
						ph += rM;
						if (ph >= L) {
							ph -= L;
							base++;
						}
					}
				}
				const uint32_t par = EPF == 2 ? (uint32_t)e0 & 1u : 0;
				uint32_t tap[DENSE_VEC], off[DENSE_VEC], w[DENSE_VEC];
				int acc[DENSE_VEC], acc1[DENSE_VEC];
#pragma unroll
				for (int i = 0; i < DENSE_VEC; i++) {
					const uint32_t f_tap = EPF == 2 ? (par ? ftap[(i + 1) / 2] : ftap[i / 2]) : ftap[i];
					const uint32_t f_off = EPF == 2 ? (par ? foff[(i + 1) / 2] : foff[i / 2]) : foff[i];
					const bool live = e0 + i < chi;         /* an element behind the row's last frame reads what is there and is zero */
					tap[i] = live ? f_tap : 0;
					off[i] = live ? f_off + (EPF == 2 && ((i + par) & 1) ? plane_len : 0) : 0;
					acc[i] = 0;
					if constexpr (WIDE) {
						w[i] = EPF == 2 ? (par ? fw[(i + 1) / 2] : fw[i / 2]) : fw[i];
						acc1[i] = 0;
					}
				}
				for (uint32_t t = 0; t < K; t++) {
#pragma unroll
					for (int i = 0; i < DENSE_VEC; i++) {
						if constexpr (WIDE) {
							const int x = xs[off[i] + t];   /* read once for both sums */
							acc[i] += (int)tab[tap[i] + t] * x;
							acc1[i] += (int)tab[tap[i] + K + t] * x;
						} else {
							acc[i] += (int)tab[tap[i] + t] * (int)xs[off[i] + t];
						}
					}
				}
#pragma unroll
				for (int i = 0; i < DENSE_VEC; i++) {
					if constexpr (WIDE)
						y[i] = e0 + i < chi ? blend(acc[i], acc1[i], w[i]) : 0;
					else
						y[i] = e0 + i < chi ? min(max((acc[i] + 8192) >> 14, -32768), 32767) : 0;
				}
			} else {
#pragma unroll
				for (int i = 0; i < DENSE_VEC; i++)
					y[i] = 0;
			}
			store_vec<false>(o + e0, y);
		}
		/* ... and the single outputs of the row's ends: [0, head) with the first pass of unit 0, [tail, sub_len) with the last of all */
		const bool front = unit == 0 && plo == bs && tid < head;
		const bool back = last && unit == units - 1 && tid >= DENSE_BLOCK - DENSE_VEC && tail + (tid - (DENSE_BLOCK - DENSE_VEC)) < sub_len;
		if (front || back) {
			const uint64_t e = front ? tid : tail + (tid - (DENSE_BLOCK - DENSE_VEC));
			int y = 0;
			if (e < chi) {
				const uint64_t j = e / EPF;
				if constexpr (WIDE) {
					const uint64_t X = j * step;
					const uint32_t frac = (uint32_t)X;
					const uint32_t off = (uint32_t)((int64_t)(X >> 32) - (int64_t)Wd + 1 - s0) + (EPF == 2 && (e & 1) ? plane_len : 0);
					y = filter_wide_one(tab + (frac >> (32 - b)) * K, xs + off, K, (frac >> (17 - b)) & 32767u);
				} else {
					const uint64_t n = j * M, base = n / L;
					const uint32_t ph = (uint32_t)(n - base * L);
					const uint32_t off = (uint32_t)((int64_t)base - (int64_t)Wd + 1 - s0) + (EPF == 2 && (e & 1) ? plane_len : 0);
					y = filter_one(tab + ph * K, xs + off, K);
				}
			}
			o[e] = to_out(o, y);
		}
		if (last)
			break;
		__syncthreads();                                         /* the next pass stages over these planes */
	}
}

} // namespace

#endif
