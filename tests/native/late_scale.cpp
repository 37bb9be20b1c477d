// Level 9's late scale (libacm_amd/csrc/acm_late_scale.h) on the host: tests/test_level9_late_scale.py builds and runs this.
//
// The last LDS pass of level 9 as pass_body (acm_kernels.hip) runs it, over two bodies of one residue class with their histories,
// written twice in plain C++:
//   plain : every stage mod 2^32, nothing scaled - the sample is (y >> 9) & 0xFFFF;
//   late  : the stages in front as the kernel has them (the 25-bit v_mad_i32_i24 forms), stage G - 2 through the injecting P forms,
//           stage G - 1 through the exact N forms of acm_late_scale.h - the sample is bytes 2..3.
// Both must agree for random 32-bit inputs and for inputs drawn from the extremes, at every position of the body (both parities of
// both stages), for a last pass of three and of two stages, with zero and non-zero histories, and the pair pack (the selector and the
// xor of acm_late_scale.h through a model of v_perm_b32) must give the words of decode.c's write-out in all four formats.
#include <stdint.h>
#include <stdio.h>

#include "acm_late_scale.h"

using namespace acm_late;

#define CHECK(c)                                                                \
	do {                                                                    \
		if (!(c)) {                                                     \
			fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
			return 1;                                               \
		}                                                               \
	} while (0)

static const int L = 9;

static const uint32_t EXTREMES[] = { 0u, 1u, 0xFFFFFFFFu, 1u << 23, 0u - (1u << 23), 1u << 24, 0u - (1u << 24), 0x7FFFFFFFu, 0x80000000u };
static const int NEXT = sizeof EXTREMES / sizeof EXTREMES[0];

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return (uint32_t)(rng_state >> 16);
}

/* the kernel's one-op forms: t - 2 z through v_mad_i32_i24 (25 bits exact), t + 2 z through v_lshl_add_u32 */
static uint32_t sub_twice24(uint32_t t, uint32_t z) { return mad_i24(z, -2, t); }
static uint32_t add_twice(uint32_t t, uint32_t z) { return (z << 1) + t; }

/* pass_body<9, 9 - G, G> without the "+1" (a last pass never starts at stage 0).  LATE: the kernel's late-scale build, else every
 * stage exact mod 2^32 and unscaled */
template <int G, bool LATE>
static void pass_body(uint32_t (&v)[2 << G], uint32_t (&h)[G][1 << G])
{
	constexpr int U = 1 << G, BODY = 2 * U, K0 = L - G;
	using Late = LateScale<L, G>;
	static_assert(Late::ON && Late::SHIFT == 7 && Late::BYTE == 2, "level 9, two or more stages");
	for (int t = 0; t < G; t++) {
		const int d = 1 << (G - 1 - t), pb = G - 1 - t;
		const bool kindN = ((L - 1 - (K0 + t)) % 2) == 0;
		uint32_t in[BODY];
		for (int u = 0; u < BODY; u++)
			in[u] = v[u];
		for (int u = 0; u < BODY; u++) {
			const uint32_t z0 = in[u];
			const uint32_t z1 = (u >= d) ? in[u - d] : h[t][u + d];
			const uint32_t z2 = (u >= 2 * d) ? in[u - 2 * d] : h[t][u];
			const int beta = (u >> pb) & 1, aneg = (u >> (pb + 1)) & 1;
			uint32_t y;
			if (LATE && t == Late::INJECT) {
				y = beta ? p_inject_odd(z0, z1, z2) : p_inject_even(z0, z1, z2);
			} else if (LATE && t == Late::EXACT) {
				y = (aneg ^ beta) == 0 ? n_exact_sub(z0, z1, z2) : n_exact_add(z0, z1, z2);
			} else if (!kindN) {
				y = beta ? (LATE ? sub_twice24(z2 + z0, z1) : z2 + z0 - 2 * z1) : add_twice(z2 + z0, z1);
			} else if ((aneg ^ beta) == 0) {
				y = LATE ? sub_twice24(z0 - z2, z1) : z0 - z2 - 2 * z1;
			} else {
				y = add_twice(z2 - z0, z1);
			}
			v[u] = y;
		}
		for (int x = 0; x < 2 * d; x++)
			h[t][x] = in[BODY - 2 * d + x];
	}
}

/* v_perm_b32 D, S0, S1, S2 for selector bytes 0..7 */
static uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel)
{
	const uint64_t both = (uint64_t)s0 << 32 | s1;
	uint32_t d = 0;
	for (int k = 0; k < 4; k++)
		d |= (uint32_t)((both >> (8 * ((sel >> (8 * k)) & 7u))) & 0xFFu) << (8 * k);
	return d;
}

/* decode.c:617-655: fmt bit 0 = big-endian, bit 1 = unsigned */
static uint32_t pcm16(uint32_t v, unsigned fmt)
{
	uint32_t w = (uint32_t)((int32_t)v >> L);
	if (fmt & 2u)
		w += 0x8000u;
	w &= 0xFFFFu;
	if (fmt & 1u)
		w = ((w & 0xFFu) << 8) | (w >> 8);
	return w;
}

static long n_samples = 0;

template <int G>
static int one_case(int mode)
{
	constexpr int U = 1 << G, BODY = 2 * U;
	uint32_t a[BODY], b[BODY], ha[G][U], hb[G][U];
	/* mode 0: a stream's first body (histories zero: `fresh` and the zeroed carry); 1: random; 2: extremes; 3: a mix; 4: all zero */
	for (int t = 0; t < G; t++)
		for (int x = 0; x < U; x++)
			ha[t][x] = hb[t][x] = 0u;
	for (int body = 0; body < 3; body++) {
		for (int u = 0; u < BODY; u++) {
			const uint32_t r = rnd();
			a[u] = b[u] = mode == 4 ? 0u : (mode == 2 || (mode == 3 && (r & 1u))) ? EXTREMES[(r >> 8) % NEXT] : rnd();
		}
		if (body == 0 && mode != 0 && mode != 4) {
			/* a warm-up body: what it leaves in the histories is what the bodies behind it see (the late build's last history in
			 * scaled units, the plain one's unscaled) */
			pass_body<G, false>(a, ha);
			pass_body<G, true>(b, hb);
			continue;
		}
		pass_body<G, false>(a, ha);
		pass_body<G, true>(b, hb);
		for (int t = 0; t + 1 < G; t++)
			for (int x = 0; x < U; x++)
				CHECK((ha[t][x] & 0x1FFFFFFu) == (hb[t][x] & 0x1FFFFFFu));      /* in front of the exact stage: unscaled, 25 bits */
		for (int u = 0; u < BODY; u++) {
			CHECK(((b[u] >> 16) & 0xFFFFu) == ((a[u] >> L) & 0xFFFFu));
			if (mode == 4)
				CHECK(b[u] == 0u);                      /* zeros stay zeros */
			n_samples++;
		}
		for (int u = 0; u < BODY; u += 2)
			for (unsigned fmt = 0; fmt < 4; fmt++) {
				const uint32_t p = perm(b[u + 1], b[u], perm_sel((uint32_t)LateScale<L, G>::BYTE, fmt & 1u)) ^ perm_flip(fmt & 1u, fmt & 2u);
				CHECK(p == (pcm16(a[u], fmt) | pcm16(a[u + 1], fmt) << 16));
			}
	}
	return 0;
}

/* each form on its own against its definition, every triple of the extremes and random triples */
static int forms()
{
	long n = 0;
	for (int i = 0; i < NEXT * NEXT * NEXT + 200000; i++) {
		const bool ex = i < NEXT * NEXT * NEXT;
		const uint32_t z0 = ex ? EXTREMES[i % NEXT] : rnd(), z1 = ex ? EXTREMES[i / NEXT % NEXT] : rnd(), z2 = ex ? EXTREMES[i / NEXT / NEXT] : rnd();
		CHECK(p_inject_even(z0, z1, z2) == (z2 + z0 + 2 * z1) << 7);
		CHECK(p_inject_odd(z0, z1, z2) == (z2 + z0 - 2 * z1) << 7);
		CHECK(n_exact_sub(z0, z1, z2) == z0 - z2 - 2 * z1);
		CHECK(n_exact_add(z0, z1, z2) == z2 - z0 + 2 * z1);
		n++;
	}
	printf("forms: %ld triples\n", n);
	return 0;
}

int main()
{
	static_assert(!LateScale<9, 1>::ON && !LateScale<8, 3>::ON && !LateScale<10, 2>::ON, "level 9 with a P stage in the last pass, nothing else");
	static_assert(LateScale<9, 3>::INJECT == 1 && LateScale<9, 3>::EXACT == 2 && LateScale<9, 2>::INJECT == 0 && LateScale<9, 2>::EXACT == 1, "stages");
	if (forms())
		return 1;
	for (int mode = 0; mode < 5; mode++)
		for (int k = 0; k < (mode == 4 ? 1 : 20000); k++)
			if (one_case<3>(mode) || one_case<2>(mode))
				return 1;
	printf("bodies: %ld samples\n", n_samples);
	return 0;
}
