// The device-free half of acm_batch_decode_windows_features under AddressSanitizer + UBSan (tests/test_dense_feat.py builds and runs
// this): g++ -fsanitize=address,undefined over acm_feat_layout.cpp alone - it links nothing else and knows no device.  The byte split
// round trip over every int16, the bounds of the four partial sums at n_fft 2048 and their join against the product itself, the
// scaling shift, the two-limb mel sum and trunc24 against a 128-bit computation, and the check, the frame count, the design, the
// layout and the grid.
#include <math.h>
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

/* y of include/acm_hip.h from E as 128 bits: the 24 leading bits through a double, which holds them exactly */
static uint32_t trunc24_ref(u128 E, uint32_t n)
{
	if (E == 0)
		return 0;
	int p = 127;
	while (!(E >> p & 1))
		p--;
	if (p > 23)
		E = E >> (p - 23) << (p - 23);
	const double hi = (double)(uint64_t)(E >> 64), lo = (double)(uint64_t)E;   /* at most 24 significant bits in one of them */
	const float y = (float)ldexp(hi * 18446744073709551616.0 + lo, -(75 - 2 * (int)n));
	uint32_t bits;
	memcpy(&bits, &y, 4);
	return bits;
}

static int split_and_join()
{
	for (int v = -32768; v <= 32767; v++) {
		const int lo = acm_feat_lo(v), hi = acm_feat_hi(v);
		CHECK(256 * hi + lo == v && lo >= -128 && lo <= 127 && hi >= -128 && hi <= 128);
		if (v >= -ACM_FEAT_WINDOW_MAX && v <= ACM_FEAT_WINDOW_MAX)
			CHECK(hi >= -127 && hi <= 127);
		if (v >= -ACM_FEAT_CS_ONE && v <= ACM_FEAT_CS_ONE)
			CHECK(hi >= -64 && hi <= 64);
	}
	CHECK(acm_feat_hi(32640) == 128);               /* why the window stops at 32639 */
	/* the four sums over 2048 terms, every term at its plane's largest magnitude: all below 2^26 */
	const int N = ACM_FEAT_MAX_FFT;
	const int64_t hh = (int64_t)N * 127 * 64, hl = (int64_t)N * 127 * 128, lh = (int64_t)N * 128 * 64, ll = (int64_t)N * 128 * 128;
	CHECK(hh < (1 << 26) && hl < (1 << 26) && lh < (1 << 26) && ll < (1 << 26));
	/* the join is the product's sum: the extremes, then random operands in range */
	for (int trial = 0; trial < 200; trial++) {
		int64_t want = 0, s[4] = {};
		for (int t = 0; t < N; t++) {
			int x, c;
			if (trial < 4) {
				x = (trial & 1) ? ACM_FEAT_WINDOW_MAX : -ACM_FEAT_WINDOW_MAX;
				c = (trial & 2) ? ACM_FEAT_CS_ONE : -ACM_FEAT_CS_ONE;
			} else {
				x = (int)(rnd() % (2 * ACM_FEAT_WINDOW_MAX + 1)) - ACM_FEAT_WINDOW_MAX;
				c = (int)(rnd() % (2 * ACM_FEAT_CS_ONE + 1)) - ACM_FEAT_CS_ONE;
			}
			want += (int64_t)x * c;
			s[0] += acm_feat_hi(x) * acm_feat_hi(c);
			s[1] += acm_feat_hi(x) * acm_feat_lo(c);
			s[2] += acm_feat_lo(x) * acm_feat_hi(c);
			s[3] += acm_feat_lo(x) * acm_feat_lo(c);
		}
		for (int k = 0; k < 4; k++)
			CHECK(s[k] > -(1 << 26) && s[k] < (1 << 26));
		CHECK(acm_feat_join((int32_t)s[0], (int32_t)s[1], (int32_t)s[2], (int32_t)s[3]) == want);
		for (uint32_t n = 7; n <= 11; n++) {
			const int64_t a = acm_feat_scale(want, n), half = (int64_t)1 << (n - 2), q = (int64_t)1 << (n - 1);
			CHECK(a * q <= want + half && want + half < (a + 1) * q);         /* floor((Re + half) / 2^q) */
		}
	}
	const int64_t top = acm_feat_scale((int64_t)N * ACM_FEAT_WINDOW_MAX * ACM_FEAT_CS_ONE, 11);
	CHECK(top <= (1 << 30) && top >= (1 << 30) - (1 << 23));
	return 0;
}

static int limbs_and_trunc24()
{
	CHECK(acm_feat_trunc24_bits(0, 0, 9) == 0);
	for (uint32_t n = 7; n <= 11; n++) {
		/* single bits of E, and the bits around them */
		for (int p = 0; p < 89; p++)
			for (int k = 0; k < 3; k++) {
				const u128 E = ((u128)1 << p) + (k == 1 && p ? ((u128)1 << p) - 1 : k == 2 && p > 24 ? (u128)1 << (p - 24) : 0);
				const uint64_t s_hi = (uint64_t)(E >> 32), s_lo = (uint64_t)E & 0xFFFFFFFFull;
				if (E >> 90)
					continue;
				CHECK(acm_feat_trunc24_bits(s_hi, s_lo, n) == trunc24_ref(E, n));
			}
	}
	for (int trial = 0; trial < 3000; trial++) {
		const uint32_t n = 7 + trial % 5, terms = trial < 5 ? 1025 : 1 + (uint32_t)(rnd() % 1025);
		const int shift = trial % 63;
		uint64_t s_hi = 0, s_lo = 0;
		u128 E = 0;
		for (uint32_t k = 0; k < terms; k++) {
			const uint64_t P = trial < 5 ? ((uint64_t)1 << 62) - 1 - k : (rnd() >> 2) >> shift;
			const uint64_t w = trial < 5 ? ACM_FEAT_W_ONE : rnd() % (ACM_FEAT_W_ONE + 1);
			s_hi += w * (P >> 32);
			s_lo += w * (P & 0xFFFFFFFFull);
			E += (u128)w * P;
		}
		CHECK(s_hi < ((uint64_t)1 << 58) && s_lo < ((uint64_t)1 << 58));
		CHECK((((u128)s_hi << 32) + s_lo) == E);
		CHECK(acm_feat_trunc24_bits(s_hi, s_lo, n) == trunc24_ref(E, n));
	}
	return 0;
}

static int check_design_layout()
{
	const uint32_t N = 512, B = 80;
	std::vector<int16_t> window(N), cs(N);
	std::vector<uint16_t> first(B), count(B);
	std::vector<uint32_t> off(B);
	size_t nw = 0;
	CHECK(acm_feat_design(16000, N, N, 160, B, 0.0, 8000.0, ACM_FEAT_CENTER, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &nw) == ACMHIP_OK);
	CHECK(nw > B && nw < (size_t)B * (N / 2 + 1));
	std::vector<uint16_t> w(nw);
	size_t again = 0;
	CHECK(acm_feat_design(16000, N, N, 160, B, 0.0, 8000.0, ACM_FEAT_CENTER, window.data(), cs.data(), first.data(), count.data(), off.data(), w.data(),
			      nw - 1, &again) == ACMHIP_ERR_ARG);
	CHECK(acm_feat_design(16000, N, N, 160, B, 0.0, 8000.0, ACM_FEAT_CENTER, window.data(), cs.data(), first.data(), count.data(), off.data(), w.data(), nw,
			      &again) == ACMHIP_OK);
	CHECK(again == nw && window[0] == 0 && window[N / 2] == ACM_FEAT_WINDOW_MAX && cs[0] == ACM_FEAT_CS_ONE && cs[N / 4] == 0 && cs[N / 2] == -ACM_FEAT_CS_ONE);
	size_t sum = 0;
	for (uint32_t b = 0; b < B; b++) {
		CHECK(off[b] == sum && count[b] >= 1 && first[b] + count[b] <= N / 2 + 1 && w[off[b]] != 0 && w[off[b] + count[b] - 1] != 0);
		sum += count[b];
	}
	CHECK(sum == nw);
	CHECK(acm_feat_design(16000, 500, 500, 160, B, 0.0, 8000.0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &again) == ACMHIP_ERR_ARG);
	CHECK(acm_feat_design(16000, N, N + 1, 160, B, 0.0, 8000.0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &again) == ACMHIP_ERR_ARG);
	CHECK(acm_feat_design(16000, N, N, 160, B, 0.0, 8000.5, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &again) == ACMHIP_ERR_ARG);
	CHECK(acm_feat_design(16000, N, N, 160, 129, 0.0, 8000.0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &again) == ACMHIP_ERR_ARG);

	acm_feat_bank bank = { N, 160, B, ACM_FEAT_CENTER, window.data(), cs.data(), first.data(), count.data(), off.data(), w.data(), 0 };
	CHECK(acm_feat_bank_check(&bank) == ACMHIP_OK && acm_feat_bank_check(nullptr) == ACMHIP_ERR_ARG);
	CHECK(acm_feat_frames(16000, &bank) == 101 && acm_feat_frames(0, &bank) == 1 && acm_feat_frames(5, nullptr) == 0);
	acm_feat_bank whole = bank;
	whole.flags = 0;
	CHECK(acm_feat_frames(511, &whole) == 0 && acm_feat_frames(512, &whole) == 1 && acm_feat_frames(512 + 159, &whole) == 1 && acm_feat_frames(512 + 160, &whole) == 2);
	{
		acm_feat_bank bad = bank;
		bad.reserved = 1;
		CHECK(acm_feat_bank_check(&bad) == ACMHIP_ERR_ARG);
		bad = bank;
		bad.flags = 4;
		CHECK(acm_feat_bank_check(&bad) == ACMHIP_ERR_ARG);
		bad = bank;
		bad.hop = N + 1;
		CHECK(acm_feat_bank_check(&bad) == ACMHIP_ERR_ARG);
		bad.hop = N;
		CHECK(acm_feat_bank_check(&bad) == ACMHIP_OK);
		std::vector<int16_t> w2 = window;
		w2[7] = ACM_FEAT_WINDOW_MAX + 1;
		bad = bank;
		bad.window = w2.data();
		CHECK(acm_feat_bank_check(&bad) == ACMHIP_ERR_ARG);
		std::vector<uint16_t> c2 = count;
		c2[B - 1] = (uint16_t)(N / 2 + 2 - first[B - 1]);
		bad = bank;
		bad.mel_count = c2.data();
		CHECK(acm_feat_bank_check(&bad) == ACMHIP_ERR_ARG);
	}

	FeatLayout L;
	const uint64_t T = 16000, nrows = 7, F = 101;
	CHECK(acm_feat_prepare(&bank, 2, T, nrows, ~0ull, &L) == ACMHIP_ERR_ARG);
	CHECK(acm_feat_prepare(&bank, 1, T, nrows, nrows * B * F - 1, &L) == ACMHIP_ERR_ARG);
	CHECK(acm_feat_prepare(&bank, 1, T, nrows, nrows * B * F, &L) == ACMHIP_OK);
	CHECK(L.n == 9 && L.F == F && L.out_words == nrows * B * F && L.n_weights == nw);
	CHECK(L.window_off() == 0 && L.cs_off() == 1024 && L.first_off() == 2048 && L.count_off() == 2048 + 160 && L.off_off() == 2048 + 320);
	CHECK(L.w_off() == 2048 + 640 && L.table_bytes() == (2048 + 640 + 2 * nw + 15) / 16 * 16);
	CHECK(L.rows_bytes() == (nrows * T + 64) * 2 && L.twiddle_off() % 256 == 0 && L.twiddle_off() >= L.rows_bytes() && L.twiddle_off() < L.rows_bytes() + 256);
	CHECK(acm_feat_bin_tiles(N) == 17 && acm_feat_twiddle_bytes(N) == (size_t)17 * 2 * 8 * 2 * 1024 && L.arena_bytes() == L.twiddle_off() + acm_feat_twiddle_bytes(N));
	std::vector<uint8_t> packed(L.table_bytes() + 1, 0xEE);
	L.pack(packed.data());
	CHECK(packed[L.table_bytes()] == 0xEE);
	CHECK(!memcmp(packed.data() + L.cs_off(), cs.data(), N * 2) && !memcmp(packed.data() + L.w_off(), w.data(), nw * 2));
	CHECK(!memcmp(packed.data() + L.off_off(), off.data(), B * 4));

	/* the grid: items are (row, tile of 16 frames), capped and strided over */
	AcmFeatGeo g = acm_feat_geo(nrows, F, 0, ACM_CAP_DENSE_GRID);
	CHECK(g.ok && g.tiles == 7 && g.nwork == 49 && g.grid == 49);
	g = acm_feat_geo(nrows, F, 3, ACM_CAP_DENSE_GRID);
	CHECK(g.ok && g.nwork == 49 && g.grid == 3);
	g = acm_feat_geo(nrows, 16, 0, ACM_CAP_DENSE_GRID);
	CHECK(g.tiles == 1 && g.grid == 7);
	g = acm_feat_geo(nrows, 17, 0, ACM_CAP_DENSE_GRID);
	CHECK(g.tiles == 2);
	g = acm_feat_geo(nrows, 0, 0, ACM_CAP_DENSE_GRID);
	CHECK(g.ok && g.nwork == 0 && g.grid == 0);
	g = acm_feat_geo(1ull << 30, 1ull << 20, 0, ACM_CAP_DENSE_GRID);
	CHECK(!g.ok);
	g = acm_feat_geo(1ull << 22, 16, 0, ACM_CAP_DENSE_GRID);
	CHECK(g.ok && g.grid == ACM_CAP_DENSE_GRID);
	return 0;
}

int main()
{
	if (split_and_join() || limbs_and_trunc24() || check_design_layout())
		return 1;
	printf("ok\n");
	return 0;
}
