// The device-free half of acm_batch_decode_windows_overlay_fir under AddressSanitizer + UBSan (tests/test_dense_fir.py builds and runs
// this): g++ -fsanitize=address,undefined over acm_fir_layout.cpp and acm_overlay_layout.cpp alone - it links nothing else and knows no
// device.  It walks every refusal of the responses with the boundary that passes beside it, lays out one accepted call and checks the
// packed taps, the filtered rows, the rewritten overlay tables and the sizes.
#include <stdio.h>

#include <vector>

#include "acm_fir_layout.h"
#include "acm_hip.h"

using namespace acmbatch;

#define CHECK(c)                                                                \
	do {                                                                    \
		if (!(c)) {                                                     \
			fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
			return 1;                                               \
		}                                                               \
	} while (0)

static acm_fir_response resp(const std::vector<int16_t> &h, uint32_t delay, uint32_t shift, uint32_t reserved = 0)
{
	return acm_fir_response{ h.data(), (uint32_t)h.size(), delay, shift, reserved };
}

int main()
{
	const size_t nwin = 6;
	const uint64_t R = 6151;
	const uint32_t NONE = ACM_FIR_NONE, TB = ACM_FIR_TAP_BLOCK;
	const std::vector<int16_t> one = { 1 }, three = { -3, 5, 7 }, edge(257, 255), block(TB, -2), more(TB + 1, 9), most(32768, 1);
	std::vector<int16_t> over = edge;
	over[256] = 256;                                        // sum |h| 65536
	std::vector<int16_t> low = edge;
	low[0] = -255;                                          // ... 65535 with a negative tap
	const std::vector<acm_fir_response> good = { resp(one, 0, 0), resp(three, 1, 15), resp(edge, 256, 30), resp(block, 0, 0), resp(more, TB, 7), resp(most, 9, 1) };
	const std::vector<uint32_t> of = { 1, NONE, 4, 1, NONE, 3 };
	acm_fir_opts fir = { good.data(), good.size(), of.data(), 0 };
	FirLayout F;

	// the check by itself
	for (const acm_fir_response &r : good)
		CHECK(acm_dense_fir_check(&r) == ACMHIP_OK);
	CHECK(acm_dense_fir_check(nullptr) == ACMHIP_ERR_ARG);
	const acm_fir_response low_r = resp(low, 0, 0), over_r = resp(over, 0, 0);
	CHECK(acm_dense_fir_check(&low_r) == ACMHIP_OK && acm_dense_fir_check(&over_r) == ACMHIP_ERR_ARG);
	std::vector<int16_t> long_h(32769, 0);
	const acm_fir_response bad[] = { resp(three, 3, 0), resp(three, 0, 31), resp(three, 0, 0, 1), resp(long_h, 0, 0), { three.data(), 0, 0, 0, 0 }, { nullptr, 3, 0, 0, 0 } };
	for (const acm_fir_response &r : bad)
		CHECK(acm_dense_fir_check(&r) == ACMHIP_ERR_ARG);
	long_h.pop_back();
	const acm_fir_response at[] = { resp(three, 2, 0), resp(three, 0, 30), resp(long_h, 32767, 0) };
	for (const acm_fir_response &r : at)
		CHECK(acm_dense_fir_check(&r) == ACMHIP_OK);

	// one accepted call: responses 1, 4 and 3 are named, in that order; 0, 2 and 5 are not, and are not packed
	CHECK(acm_fir_prepare(&fir, nwin, &F) == ACMHIP_OK);
	CHECK(F.nfilt() == 4 && F.slot == (std::vector<uint32_t>{ 6, 1, 7, 8, 4, 9 }));
	CHECK(F.taps.size() == TB + 2 * TB + TB && F.taps_bytes() % 128 == 0 && F.rows_off() == F.taps_bytes() && F.table_bytes() == F.taps_bytes() + 4 * 24);
	CHECK(F.rows[0].src == 0 && F.rows[0].dst == 6 && F.rows[0].taps_off == 0 && F.rows[0].nblk == 1 && F.rows[0].lead == -1 && F.rows[0].shift == 15);
	CHECK(F.rows[1].src == 2 && F.rows[1].dst == 7 && F.rows[1].taps_off == TB / 2 && F.rows[1].nblk == 2 && F.rows[1].lead == 0 && F.rows[1].shift == 7);
	CHECK(F.rows[2].src == 3 && F.rows[2].dst == 8 && F.rows[2].taps_off == 0 && F.rows[2].nblk == 1);              // response 1 again: packed once
	CHECK(F.rows[3].src == 5 && F.rows[3].dst == 9 && F.rows[3].taps_off == 3 * TB / 2 && F.rows[3].nblk == 1 && F.rows[3].lead == -(int)(TB - 1));
	CHECK(F.taps[0] == 7 && F.taps[1] == 5 && F.taps[2] == -3 && F.taps[3] == 0 && F.taps[TB - 1] == 0);            // reversed, zeros behind
	CHECK(F.taps[TB] == 9 && F.taps[2 * TB] == 9 && F.taps[2 * TB + 1] == 0 && F.taps[3 * TB] == -2 && F.taps[4 * TB - 1] == -2);

	// the overlay's tables seen through it: the caller's records are not touched
	std::vector<acm_overlay_row> rows = { { 0, ACM_OVERLAY_NONE, 0, 0, 0, 0, 0, 0 }, { 1, 2, 4096, 655360, 0, 0, 0, 0 }, { 3, 3, 4096, 1, 0, 0, 0, 0 },
					      { 4, 5, 4096, 0, 100, 0, 0, 0 }, { 5, 1, 4096, 65536, 0, 0, 0, 0 } };
	OverlayLayout O;
	CHECK(acm_overlay_prepare(rows.data(), rows.size(), nwin, R, rows.size() * R, &O) == ACMHIP_OK);
	CHECK(O.marked == (std::vector<uint32_t>{ 1, 2, 3, 5 }) && O.src_arena_words() == nwin * R + 64);
	acm_fir_remap(F, &O);
	CHECK(O.nsrc == 10 && O.src_arena_words() == 10 * R + 64 && O.energy_bytes() == 80);
	CHECK(O.marked == (std::vector<uint32_t>{ 1, 7, 8, 9 }));
	CHECK(O.rows[0].a == 6 && O.rows[0].b == ACM_OVERLAY_NONE && O.rows[1].a == 1 && O.rows[1].b == 7 && O.rows[2].a == 8 && O.rows[2].b == 8);
	CHECK(O.rows[3].a == 4 && O.rows[3].b == 9 && O.rows[4].a == 9 && O.rows[4].b == 1);
	CHECK(rows[0].a == 0 && rows[1].b == 2 && rows[2].a == 3 && rows[4].a == 5);

	// nothing to filter: no opts, no responses, no window that names one - the overlay's layout stays what it was
	const std::vector<uint32_t> none(nwin, NONE);
	acm_fir_opts idle = { good.data(), good.size(), none.data(), 0 }, empty = { nullptr, 0, nullptr, 0 };
	for (const acm_fir_opts *o : { (const acm_fir_opts *)nullptr, (const acm_fir_opts *)&idle, (const acm_fir_opts *)&empty }) {
		CHECK(acm_fir_prepare(o, nwin, &F) == ACMHIP_OK && F.nfilt() == 0 && F.taps.empty() && F.table_bytes() == 0);
		OverlayLayout P;
		CHECK(acm_overlay_prepare(rows.data(), rows.size(), nwin, R, rows.size() * R, &P) == ACMHIP_OK);
		acm_fir_remap(F, &P);
		CHECK(P.nsrc == nwin && P.marked == (std::vector<uint32_t>{ 1, 2, 3, 5 }) && P.rows[0].a == 0);
	}

	// the refusals
	acm_fir_opts t = fir;
	t.responses = nullptr;
	CHECK(acm_fir_prepare(&t, nwin, &F) == ACMHIP_ERR_ARG);
	t = fir;
	t.of_window = nullptr;
	CHECK(acm_fir_prepare(&t, nwin, &F) == ACMHIP_ERR_ARG);
	t = fir;
	t.reserved = 1;
	CHECK(acm_fir_prepare(&t, nwin, &F) == ACMHIP_ERR_ARG);
	t = fir;
	t.nresp = 65537;
	CHECK(acm_fir_prepare(&t, nwin, &F) == ACMHIP_ERR_ARG);
	std::vector<uint32_t> of2 = of;
	of2[4] = (uint32_t)good.size();                         // an entry == nresp
	t = fir;
	t.of_window = of2.data();
	CHECK(acm_fir_prepare(&t, nwin, &F) == ACMHIP_ERR_ARG);
	of2[4] = (uint32_t)good.size() - 1;
	CHECK(acm_fir_prepare(&t, nwin, &F) == ACMHIP_OK && F.nfilt() == 5);
	of2[4] = NONE - 1;
	CHECK(acm_fir_prepare(&t, nwin, &F) == ACMHIP_ERR_ARG);
	for (const acm_fir_response &r : bad) {                 // a response that fails the check, named or not
		std::vector<acm_fir_response> rs = good;
		rs[0] = r;
		t = fir;
		t.responses = rs.data();
		CHECK(acm_fir_prepare(&t, nwin, &F) == ACMHIP_ERR_ARG);
	}
	// 2^22 taps in the named responses: 128 of 32768 pass, one tap more does not; unnamed ones do not count
	std::vector<acm_fir_response> many(130, resp(most, 0, 0));
	many[128] = resp(one, 0, 0);
	std::vector<uint32_t> all(128);
	for (uint32_t k = 0; k < 128; k++)
		all[k] = k;
	acm_fir_opts big = { many.data(), many.size(), all.data(), 0 };
	CHECK(acm_fir_prepare(&big, all.size(), &F) == ACMHIP_OK && F.taps.size() == (1u << 22) && F.nfilt() == 128);
	all.push_back(128);
	big.of_window = all.data();
	CHECK(acm_fir_prepare(&big, all.size(), &F) == ACMHIP_ERR_ARG);
	all.back() = 5;                                         // a response named twice counts once
	CHECK(acm_fir_prepare(&big, all.size(), &F) == ACMHIP_OK && F.nfilt() == 129);
	printf("ok\n");
	return 0;
}
