// The integer logarithm of acm_batch_decode_windows_logmel under AddressSanitizer + UBSan (tests/test_dense_logmel.py builds and runs
// this): g++ -fsanitize=address,undefined over acm_feat_layout.cpp alone - it links nothing else and knows no device.
// acm_feat_log_q16 against the contract's text on 128 bits - the leading bit, the 24 leading bits, sixteen squarings - at the ends of
// E's range and astride the carry of its two limbs, acm_feat_log_out against the scale's text, the linear feature's bits against the
// same mantissa, the check at its boundaries, and the layout's table of maxima.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "acm_feat_layout.h"
#include "acm_hip.h"

using namespace acmbatch;
typedef unsigned __int128 u128;

#define CHECK(c)                                                                \
	do {                                                                    \
		if (!(c)) {                                                     \
			fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
			return 1;                                               \
		}                                                               \
	} while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return rng_state;
}

/* L of include/acm_hip.h from E as 128 bits, line by line */
static int64_t log_ref(u128 E, uint32_t n, int64_t floor_q16, uint32_t *mant)
{
	*mant = 0;
	if (E == 0)
		return floor_q16;
	int p = 127;
	while (!(E >> p & 1))
		p--;
	const u128 m = p > 23 ? E >> (p - 23) : E << (23 - p);
	*mant = (uint32_t)m;
	u128 x = m;
	int64_t frac = 0;
	for (int i = 0; i < 16; i++) {
		x = x * x;
		if (x >= (u128)1 << 47) {
			frac = frac * 2 + 1;
			x >>= 24;
		} else {
			frac = frac * 2;
			x >>= 23;
		}
		if (x < (u128)1 << 23 || x >= (u128)1 << 24)
			return INT64_MIN;
	}
	const int64_t L = ((int64_t)p - (75 - 2 * (int64_t)n)) * 65536 + frac;
	return L > floor_q16 ? L : floor_q16;
}

/* one E at one n: the two limbs as the kernel's sums hold them (s_lo up to 58 bits wide, so the same E in several splits) */
static int one(u128 E, uint32_t n)
{
	const int32_t floors[3] = { -ACM_FEAT_LOG_FLOOR_MAX, -2177059, 5 * 65536 };
	for (int split = 0; split < 3; split++) {
		/* s_lo takes `extra` more of E than its low 32 bits, as far as E has them */
		const u128 extra = split == 0 ? 0 : split == 1 ? (E >> 32) & 0x3FFFFFFu : (E >> 32) & 1u;
		const uint64_t s_hi = (uint64_t)((E >> 32) - extra), s_lo = (uint64_t)(E & 0xFFFFFFFFu) + (uint64_t)(extra << 32);
		CHECK((((u128)s_hi << 32) + s_lo) == E && s_hi < ((uint64_t)1 << 58) && s_lo < ((uint64_t)1 << 58));
		for (int f = 0; f < 3; f++) {
			uint32_t mant;
			const int64_t want = log_ref(E, n, floors[f], &mant);
			CHECK(want != INT64_MIN);
			CHECK(acm_feat_log_q16(s_hi, s_lo, n, floors[f]) == want);
			/* the linear feature keeps the same mantissa */
			const uint32_t lin = acm_feat_trunc24_bits(s_hi, s_lo, n);
			CHECK(E == 0 ? lin == 0 : (lin & 0x7FFFFFu) == (mant & 0x7FFFFFu));
			uint32_t m2;
			const int p = acm_feat_lead(s_hi, s_lo, &m2);
			CHECK(E == 0 ? p == -1 : (m2 == mant && (int)(lin >> 23) == p - (75 - 2 * (int)n) + 127));
		}
	}
	return 0;
}

static int logarithm()
{
	const u128 one128 = 1;
	/* the largest E the bounds allow: 1025 bins of weight 32768 and P = 2^62 - 1 */
	const u128 top = (u128)1025 * 32768 * (((u128)1 << 62) - 1);
	CHECK(top < one128 << 89);
	std::vector<u128> es = { 0, 1, 2, 3, (one128 << 23) - 1, one128 << 23, (one128 << 23) + 1, (one128 << 24) - 1, one128 << 24, (one128 << 24) + 1,
				 /* astride the carry of (s_hi << 32) + s_lo into the high word, and of the low limb into the high one */
				 (one128 << 32) - 1, one128 << 32, (one128 << 32) + 1, (one128 << 58) - 1, one128 << 58, (one128 << 63) - 1, one128 << 63,
				 (one128 << 64) - 1, one128 << 64, (one128 << 64) + 1, (one128 << 64) + ((one128 << 41) - 1), (one128 << 87) - 1, one128 << 87,
				 (one128 << 88) + ((one128 << 65) - 1), top, top - 1 };
	for (int p = 0; p < 89; p++) {
		es.push_back(one128 << p);
		es.push_back((one128 << p) | (one128 << p) >> 1 | 1);
		es.push_back((one128 << (p + 1)) - 1 < top ? (one128 << (p + 1)) - 1 : top);
	}
	for (int trial = 0; trial < 4000; trial++) {
		const u128 v = ((u128)rnd() << 64 | rnd()) >> (39 + trial % 89);
		es.push_back(v < top ? v : top);
	}
	for (size_t i = 0; i < es.size(); i++) {
		if (one(es[i], 7) || one(es[i], 11) || (i % 3 == 0 && one(es[i], 9)))
			return 1;
	}
	/* the ends of the fraction, and the largest and the least L of any bank */
	CHECK(acm_feat_log_frac(1u << 23) == 0 && acm_feat_log_frac((1u << 24) - 1) == 65535);
	CHECK(acm_feat_log_q16(0, 1, 7, -ACM_FEAT_LOG_FLOOR_MAX) == -61 * 65536 && acm_feat_log_q16(0, 1, 11, -ACM_FEAT_LOG_FLOOR_MAX) == -53 * 65536);
	CHECK(acm_feat_log_q16((uint64_t)(top >> 32), (uint64_t)(top & 0xFFFFFFFFu), 11, 0) < 36 * 65536);
	CHECK(acm_feat_log_q16(0, 0, 9, 77) == 77 && acm_feat_log_q16(0, 0, 9, -ACM_FEAT_LOG_FLOOR_MAX) == -ACM_FEAT_LOG_FLOOR_MAX);
	uint32_t last = 0;
	for (uint32_t m = 1u << 23; m < 1u << 24; m += 251) {           /* monotone (every mantissa: tests/test_dense_logmel.py) */
		const uint32_t f = acm_feat_log_frac(m);
		CHECK(f >= last && f <= 65535);
		last = f;
	}
	return 0;
}

static uint32_t float_bits(float y)
{
	uint32_t b;
	memcpy(&b, &y, 4);
	return b;
}

static int scale()
{
	/* V on 128 bits with a floor division, and the float as a quotient of two exact doubles */
	const int32_t ls[] = { 0, 1, -1, 65536, -65536, 62 * 65536, -62 * 65536, ACM_FEAT_LOG_FLOOR_MAX, -ACM_FEAT_LOG_FLOOR_MAX, -2177059, 123457, -7 };
	const uint32_t muls[] = { 1, 2, 1u << 23, (1u << 23) + 1, 1u << 24, 1262611, 11629080, 50504453, 65000000 };
	const int32_t offs[] = { 0, 1, -1, 65536, -12345, 3000000, -3000000 };
	for (int32_t l : ls)
		for (uint32_t mul : muls)
			for (int32_t off : offs) {
				const __int128 t = (__int128)l * mul + ((__int128)1 << 23);
				const __int128 q = (t - (((t % ((__int128)1 << 24)) + ((__int128)1 << 24)) % ((__int128)1 << 24))) / ((__int128)1 << 24);
				const int64_t v = (int64_t)q + off;
				if (v <= -(1 << 24) || v >= (1 << 24))
					continue;
				CHECK(acm_feat_log_out(l, mul, off) == float_bits((float)((double)v / 65536.0)));
				CHECK((double)(float)((double)v / 65536.0) == (double)v / 65536.0);             /* exact */
			}
	CHECK(acm_feat_log_out(0, 1u << 24, 0) == 0);                    /* +0.0, every bit */
	CHECK(acm_feat_log_out(65536, 1u << 24, 0) == float_bits(1.0f) && acm_feat_log_out(-65536, 1u << 24, 0) == float_bits(-1.0f));
	CHECK(acm_feat_log_out(-1, 1u << 23, 0) == 0 && acm_feat_log_out(-3, 1u << 23, 0) == float_bits(-1.0f / 65536.0f));   /* the shift floors */
	return 0;
}

static int check_and_layout()
{
	const uint32_t N = 128;
	std::vector<int16_t> window(N, 1), cs(N, 1);
	uint16_t first = 0, count = 1, w = 1;
	uint32_t off = 0;
	acm_feat_bank bank = { N, 64, 1, 0, window.data(), cs.data(), &first, &count, &off, &w, 0 };
	const acm_feat_log good = { ACM_FEAT_LOG_TOP, -2177059, 1262611, 65536, 1741647, 0 };
	CHECK(acm_feat_log_check(&bank, &good) == ACMHIP_OK);
	CHECK(acm_feat_log_check(&bank, nullptr) == ACMHIP_ERR_ARG && acm_feat_log_check(nullptr, &good) == ACMHIP_ERR_ARG);
	acm_feat_bank bad_bank = bank;
	bad_bank.flags = 4;
	CHECK(acm_feat_log_check(&bad_bank, &good) == ACMHIP_ERR_ARG);
	acm_feat_log g = good;
	g.flags = 3;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_ERR_ARG);
	g = good;
	g.reserved = 1;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_ERR_ARG);
	g = good;
	g.flags = 0;                                                    /* a top without the flag */
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_ERR_ARG);
	g.top_q16 = 0;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_OK);
	g = good;
	g.top_q16 = ACM_FEAT_LOG_TOP_MAX;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_OK);
	g.top_q16 = ACM_FEAT_LOG_TOP_MAX + 1;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_ERR_ARG);
	g = good;
	g.floor_q16 = -ACM_FEAT_LOG_FLOOR_MAX;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_OK);
	g.floor_q16 = -ACM_FEAT_LOG_FLOOR_MAX - 1;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_ERR_ARG);
	g.floor_q16 = ACM_FEAT_LOG_FLOOR_MAX;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_OK);
	g.floor_q16 = ACM_FEAT_LOG_FLOOR_MAX + 1;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_ERR_ARG);
	g = good;
	g.mul_q24 = 0;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_ERR_ARG);
	g.mul_q24 = 1;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_OK);
	/* the bound: Lb = 62 * 65536, ((Lb * mul) >> 24) + |offset| + 1 < 2^24 */
	g = good;
	g.mul_q24 = 1u << 24;
	g.offset_q16 = (1 << 24) - 62 * 65536 - 2;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_OK);
	g.offset_q16 = -g.offset_q16;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_OK);
	g.offset_q16 = (1 << 24) - 62 * 65536 - 1;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_ERR_ARG);
	g.offset_q16 = -g.offset_q16;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_ERR_ARG);
	g.offset_q16 = INT32_MIN;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_ERR_ARG);
	g = good;
	g.offset_q16 = 0;
	g.mul_q24 = ACM_FEAT_LOG_MUL_MAX;                               /* 2^28: 62 * 16 * 65536 is past 2^24 */
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_ERR_ARG);
	g.mul_q24 = ACM_FEAT_LOG_MUL_MAX + 1;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_ERR_ARG);
	g.floor_q16 = -ACM_FEAT_LOG_FLOOR_MAX;                          /* the floor takes Lb over: 64 * 65536 * mul >> 24 */
	g.mul_q24 = (1u << 26) - 17;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_OK);
	g.mul_q24 = 1u << 26;
	CHECK(acm_feat_log_check(&bank, &g) == ACMHIP_ERR_ARG);

	/* the layout: the maxima behind the operand on a multiple of 256, with ACM_FEAT_LOG_TOP alone */
	FeatLayout plain, log, top;
	const uint64_t T = 2100, nrows = 7;
	CHECK(acm_feat_prepare(&bank, 1, T, nrows, ~0ull, &plain) == ACMHIP_OK && !plain.has_log && !plain.top() && plain.rowmax_bytes() == 0);
	g = good;
	g.flags = 0;
	g.top_q16 = 0;
	CHECK(acm_feat_prepare(&bank, &g, 1, T, nrows, ~0ull, &log) == ACMHIP_OK && log.has_log && !log.top() && log.rowmax_bytes() == 0);
	CHECK(log.arena_bytes() == plain.arena_bytes() && log.table_bytes() == plain.table_bytes() && log.out_words == plain.out_words);
	CHECK(acm_feat_prepare(&bank, &good, 1, T, nrows, ~0ull, &top) == ACMHIP_OK && top.has_log && top.top() && top.log.top_q16 == good.top_q16);
	CHECK(top.table_bytes() == plain.table_bytes() && top.twiddle_off() == plain.twiddle_off());
	CHECK(top.rowmax_off() % 256 == 0 && top.rowmax_off() >= plain.arena_bytes() && top.rowmax_off() < plain.arena_bytes() + 256);
	CHECK(top.rowmax_bytes() == nrows * 4 && top.arena_bytes() == top.rowmax_off() + nrows * 4);
	CHECK(acm_feat_prepare(&bank, nullptr, 1, T, nrows, ~0ull, &top) == ACMHIP_ERR_ARG);
	CHECK(acm_feat_prepare(&bank, &good, 2, T, nrows, ~0ull, &top) == ACMHIP_ERR_ARG);
	CHECK(acm_feat_prepare(&bank, &good, 1, T, nrows, plain.out_words - 1, &top) == ACMHIP_ERR_ARG);
	return 0;
}

int main()
{
	if (logarithm() || scale() || check_and_layout())
		return 1;
	printf("ok\n");
	return 0;
}
