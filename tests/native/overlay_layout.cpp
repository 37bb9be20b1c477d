// The device-free half of acm_batch_decode_windows_overlay under AddressSanitizer + UBSan (tests/test_dense_overlay.py builds and runs
// this): g++ -fsanitize=address,undefined over acm_overlay_layout.cpp alone - it links nothing else and knows no device.  It walks
// every refusal of the row table, lays out one accepted table and checks its records, its list of rows to sum and its sizes, and
// holds the gain to its extremes.
#include <stdio.h>

#include <vector>

#include "acm_hip.h"
#include "acm_overlay_layout.h"

using namespace acmbatch;

#define CHECK(c)                                                                \
	do {                                                                    \
		if (!(c)) {                                                     \
			fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
			return 1;                                               \
		}                                                               \
	} while (0)

static acm_overlay_row row(uint32_t a, uint32_t b, uint32_t vol, uint32_t snr, uint32_t gain, uint32_t reserved = 0)
{
	return acm_overlay_row{ a, b, vol, snr, gain, reserved, 0, 0 };
}

int main()
{
	const size_t nwin = 6;
	const uint64_t R = 6151;
	OverlayLayout O;
	const std::vector<acm_overlay_row> good = { row(0, ACM_OVERLAY_NONE, 0, 0, 0),      row(5, 2, 4096, 655360, 77), row(2, 2, 65535, 1, 0),
						    row(1, 3, 1, 0, 32768),                 row(4, 2, 2048, 0xFFFFFFFFu, 0), row(0, ACM_OVERLAY_NONE, 2048, 9, 40000) };
	// one accepted table
	CHECK(acm_overlay_prepare(good.data(), good.size(), nwin, R, good.size() * R, &O) == ACMHIP_OK);
	CHECK(O.rows.size() == good.size() && O.nsrc == nwin && O.row_words == R && O.out_words == good.size() * R);
	CHECK(O.marked == (std::vector<uint32_t>{ 2, 4, 5 }));
	CHECK(O.rows[0].vol == 4096 && O.rows[0].b == ACM_OVERLAY_NONE && O.rows[0].snr == 0 && O.rows[0].gain == 0);
	CHECK(O.rows[1].snr == 655360 && O.rows[1].gain == 0 && O.rows[3].snr == 0 && O.rows[3].gain == 32768 && O.rows[3].vol == 1);
	CHECK(O.rows[5].snr == 0 && O.rows[5].gain == 0);                // nothing is laid over it: neither is read
	CHECK(O.src_arena_words() == nwin * R + 64);
	CHECK(O.upload_bytes() == 6 * 24 + 16 && O.energy_off() == O.upload_bytes() && O.energy_bytes() == nwin * 8);
	CHECK(O.result_off() == O.energy_off() + O.energy_bytes() && O.result_bytes() == 6 * 24 && O.table_bytes() == O.result_off() + O.result_bytes());
	// no rows at all: nothing to write, sources alone
	CHECK(acm_overlay_prepare(nullptr, 0, nwin, R, 0, &O) == ACMHIP_OK && O.rows.empty() && O.marked.empty() && O.upload_bytes() == 0);

	// the refusals
	CHECK(acm_overlay_prepare(nullptr, 3, nwin, R, 3 * R, &O) == ACMHIP_ERR_ARG);
	CHECK(acm_overlay_prepare(good.data(), good.size(), nwin, R, good.size() * R - 1, &O) == ACMHIP_ERR_ARG);
	CHECK(acm_overlay_prepare(good.data(), good.size(), nwin, 1ull << 24, ~0ull, &O) == ACMHIP_ERR_ARG);
	CHECK(acm_overlay_prepare(good.data(), good.size(), nwin, (1ull << 24) - 1, ~0ull, &O) == ACMHIP_OK);
	CHECK(acm_overlay_prepare(good.data(), good.size(), 5, R, ~0ull, &O) == ACMHIP_ERR_ARG);          // a == nwin
	const acm_overlay_row bad[] = { row(6, ACM_OVERLAY_NONE, 0, 0, 0), row(0, 6, 0, 0, 0),     row(0, 0xFFFFFFFEu, 0, 1, 0), row(0, 1, 0, 0, 32769),
					row(0, 1, 0, 0, 0, 1),             row(0, 1, 65536, 0, 0), row(0xFFFFFFFFu, 1, 0, 0, 0) };
	for (const acm_overlay_row &b : bad) {
		std::vector<acm_overlay_row> t = good;
		t.push_back(b);
		CHECK(acm_overlay_prepare(t.data(), t.size(), nwin, R, ~0ull, &O) == ACMHIP_ERR_ARG);
		t.back() = row(0, 1, 0, 5, 32769);              // SNR mode: `gain` is not read
		CHECK(acm_overlay_prepare(t.data(), t.size(), nwin, R, ~0ull, &O) == ACMHIP_OK && O.rows.back().gain == 0);
	}

	// the gain at its ends
	CHECK(acm_dense_overlay_gain(0, 5, 65536) == 0 && acm_dense_overlay_gain(5, 0, 65536) == 0 && acm_dense_overlay_gain(5, 5, 0) == 0);
	CHECK(acm_dense_overlay_gain(1000, 1000, 65536) == 4096 && acm_dense_overlay_gain(1000, 1000, 1) == 32768);
	CHECK(acm_dense_overlay_gain(~0ull, ~0ull, 0xFFFFFFFFu) == 16 && acm_dense_overlay_gain(~0ull, 1, 1) == 32768);
	CHECK(acm_dense_overlay_gain(1, ~0ull, 0xFFFFFFFFu) == 0 && acm_dense_overlay_gain(64, 1, 65536) == 32768 && acm_dense_overlay_gain(63, 1, 65536) == 32510);
	printf("ok\n");
	return 0;
}
