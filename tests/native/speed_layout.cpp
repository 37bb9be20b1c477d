// The device-free half of ACM_DENSE_SPEED under AddressSanitizer + UBSan (tests/test_dense_speed.py builds and runs this):
// g++ -fsanitize=address,undefined over acm_resample_layout.cpp, acm_dense_layout.cpp and what they link (acm_window_layout.cpp,
// acm_kernel_geo.cpp); nothing here knows a device.  It walks the classification set of the contract, designs every wide table, lays
// out a call of exact, wide, plain and turned-away rows into tables of exactly the size the layout asks for, and has the 17th
// table refused.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "acm_dense_layout.h"
#include "acm_hip.h"

using namespace acmbatch;

#define CHECK(c)                                                                \
	do {                                                                    \
		if (!(c)) {                                                     \
			fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
			return 1;                                               \
		}                                                               \
	} while (0)

static WindowItem item_at(uint32_t rate)
{
	WindowItem it;
	it.info.channels = 1;
	it.info.rate = rate;
	it.info.rows = 16;
	it.info.cols = 32;
	it.info.total_values = 1u << 20;
	it.len = 1u << 20;
	it.ok = true;
	it.whole = 1u << 20;
	return it;
}

static acm_batch_window window(uint32_t item, uint64_t first, uint64_t words, uint32_t num, uint32_t den)
{
	acm_batch_window w{};
	w.item = item;
	w.first_word = first;
	w.max_words = words;
	w.reserved = num << 16 | den;
	return w;
}

int main()
{
	// the classification set
	struct { uint32_t ri, ro, num, den; int kind; uint32_t c, K, P; } set[] = {
		{ 22050, 16000, 9, 10, SPEED_WIDE, 51, 22, 512 },  { 22050, 16000, 11, 10, SPEED_WIDE, 42, 26, 512 },
		{ 44100, 16000, 11, 10, SPEED_WIDE, 21, 50, 256 }, { 22050, 22050, 9, 10, SPEED_EXACT, 0, 16, 0 },
		{ 22051, 22050, 1, 1, SPEED_WIDE, 63, 18, 512 },   { 16000, 16000, 1001, 1000, SPEED_WIDE, 63, 18, 512 },
		{ 22050, 2450, 1, 1, SPEED_BAD, 0, 0, 0 },         { 22050, 22050, 9, 1, SPEED_BAD, 0, 0, 0 },
		{ 22050, 22050, 7, 7, SPEED_NONE, 0, 16, 0 },      { 16000, 2050, 999, 1000, SPEED_WIDE, 8, 128, 64 },
		{ 8000, 4294967291u, 65535, 65534, SPEED_BAD, 0, 0, 0 }, { 0, 22050, 1, 1, SPEED_BAD, 0, 0, 0 },
	};
	for (const auto &s : set) {
		const SpeedFilter f = acm_speed_filter(s.ri, s.ro, s.num, s.den);
		CHECK(f.kind == s.kind && f.c == s.c && f.K == s.K && f.P == s.P);
		acm_dense_speed_info info;
		const int rc = acm_dense_speed_taps(s.ri, s.ro, s.num, s.den, &info, nullptr, 0);
		CHECK((rc == ACMHIP_OK) == (s.kind != SPEED_BAD));
		if (rc != ACMHIP_OK) {
			CHECK(acm_dense_speed_frames(1000, s.ri, s.ro, s.num, s.den) == UINT64_MAX);
			continue;
		}
		std::vector<int16_t> taps((size_t)info.phases * info.K);
		CHECK(acm_dense_speed_taps(s.ri, s.ro, s.num, s.den, nullptr, taps.data(), taps.size()) == ACMHIP_OK);
		CHECK(acm_dense_speed_taps(s.ri, s.ro, s.num, s.den, nullptr, taps.data(), taps.size() - 1) == ACMHIP_ERR_ARG);
		for (uint32_t p = 0; p < info.phases; p++) {
			long sum = 0;
			for (uint32_t t = 0; t < info.K; t++)
				sum += taps[(size_t)p * info.K + t];
			CHECK(sum == 16384);
		}
		CHECK(acm_dense_speed_frames(1ull << 50, s.ri, s.ro, s.num, s.den) != UINT64_MAX);
	}
	for (uint32_t c = 8; c <= 64; c++) {
		const auto tab = acm_wide_table(c);
		CHECK(tab && tab->wide && tab->q.size() == (size_t)(tab->P + 1) * tab->r.K && tab->q.size() <= ACM_RESAMPLE_MAX_TAPS);
	}
	CHECK(!acm_wide_table(7) && !acm_wide_table(65));
	// a window far too long: the check multiplies in 128 bits
	CHECK(acm_resample_frames(~0ull, 0x7FFFFFFF, 1) == UINT64_MAX && acm_resample_frames(~0ull, 3, 3) == ~0ull);

	// one call: exact, wide, plain and turned-away rows; then tables until the 17th is refused
	const uint32_t rates[] = { 22050, 11025, 44100, 16000, 7350, 66150, 4410, 110250, 14700, 33075, 8820, 55125, 13230, 36750, 3675, 3150, 154350, 22051 };
	std::vector<WindowItem> items;
	for (uint32_t r : rates)
		items.push_back(item_at(r));
	acm_batch_opts opts{};
	opts.fmt = ACMHIP_FMT_S16LE;
	opts.d_pcm = reinterpret_cast<int16_t *>(0x1000);
	acm_dense_opts dense{ 64, 1, ACM_DENSE_RESAMPLE | ACM_DENSE_SPEED, 22050, 0 };
	std::vector<acm_batch_window> wins = { window(0, 8, 40, 9, 10), window(0, 3, 50, 29999, 30000), window(0, 0, 64, 0, 0), window(1, 5, 30, 1001, 1000),
					       window(2, 1, 100, 1, 1), window(17, 9, 60, 0, 0), window(2, 0, 8, 5, 1), window(99, 0, 4, 9, 10) };
	opts.d_pcm_words = 64 * 64;
	DenseLayout D;
	CHECK(acm_dense_prepare(items.data(), items.size(), wins.data(), wins.size(), opts, &dense, &D) == ACMHIP_OK);
	CHECK(D.tables.size() == 4 && D.has_wide() && D.rejected[6] && D.bad_ratio[6] && !D.rejected[7]);
	std::vector<WindowSlot> slots(wins.size());
	for (size_t k = 0; k < wins.size(); k++) {
		slots[k].active = D.wins[k].max_words != 0 && wins[k].item < items.size();
		slots[k].words = slots[k].active ? D.wins[k].max_words : 0;
		slots[k].dev_off = 64 * k;
		wins[k].words = slots[k].words;
	}
	std::vector<AcmDenseRow> rows(wins.size());
	CHECK(!acm_dense_rows(D, slots.data(), wins.data(), rows.data()));
	CHECK(acm_dense_wide_rows(D, rows.data()));
	CHECK(D.table_bytes() == wins.size() * (sizeof(AcmDenseRow) + sizeof(AcmSpeedRow)) + D.tap_at(D.tables.size()) * sizeof(int16_t));
	std::vector<AcmSpeedRow> sp(wins.size());
	std::vector<int16_t> taps(D.tap_at(D.tables.size()));
	acm_dense_speed_rows(D, rows.data(), sp.data(), taps.data());
	CHECK(sp[0].L == 10 && sp[0].M == 9 && !sp[0].wide && sp[0].n_out == 45);
	CHECK(sp[1].wide && sp[1].b == 9 && sp[1].Wd == 8 && sp[1].n_out == 51 && sp[1].step == ((29999ull << 32) / 30000));
	CHECK(sp[2].L == 0 && sp[3].wide && sp[4].L == 1 && sp[4].M == 2 && sp[5].wide && sp[5].tab != sp[1].tab && sp[6].L == 0 && sp[7].L == 0);
	// the one decision the driver and the visitors take: the same three tables into a region of exactly table_bytes(), all of it goes up
	std::vector<uint8_t> table(D.table_bytes());
	DenseLaunch launch = acm_dense_tables(D, slots.data(), wins.data(), table.data());
	CHECK(launch.kernel == DENSE_SPEED && launch.bytes == D.table_bytes());
	CHECK(!memcmp(table.data(), rows.data(), D.row_table_bytes()) && !memcmp(table.data() + D.resample_off(), sp.data(), sp.size() * sizeof(AcmSpeedRow)) &&
	      !memcmp(table.data() + D.taps_off(), taps.data(), taps.size() * sizeof(int16_t)));
	// ... where staging left nothing of the wide rows the call goes on as without the flag
	for (size_t k : { 1, 3, 5 })
		wins[k].words = 0;
	acm_dense_rows(D, slots.data(), wins.data(), rows.data());
	CHECK(!acm_dense_wide_rows(D, rows.data()));
	std::vector<AcmResampleRow> rs(wins.size());
	CHECK(acm_dense_resample_rows(D, rows.data(), rs.data(), taps.data()) && rs[0].L == 10 && rs[1].L == 0 && rs[4].M == 2);
	launch = acm_dense_tables(D, slots.data(), wins.data(), table.data());
	CHECK(launch.kernel == DENSE_RESAMPLE && launch.bytes == D.table_bytes());
	CHECK(!memcmp(table.data() + D.resample_off(), rs.data(), rs.size() * sizeof(AcmResampleRow)));
	// ... and where it left nothing of any filtered row, the row table alone goes up, for the kernel of a call without the flags
	for (size_t k : { 0, 4 })
		wins[k].words = 0;
	launch = acm_dense_tables(D, slots.data(), wins.data(), table.data());
	CHECK(launch.kernel == DENSE_PLAIN && launch.bytes == D.row_table_bytes());

	// 14 exact tables and two wide ones are 16; one more of either kind is refused
	wins.clear();
	for (uint32_t k = 1; k <= 14; k++)
		wins.push_back(window(k, 0, 8, 0, 0));
	wins.push_back(window(0, 0, 8, 29999, 30000));
	wins.push_back(window(0, 0, 8, 1001, 1000));
	CHECK(acm_dense_prepare(items.data(), items.size(), wins.data(), wins.size(), opts, &dense, &D) == ACMHIP_OK && D.tables.size() == 16);
	wins.push_back(window(3, 0, 8, 29999, 30000));          // c = 64 again: a table the call has
	CHECK(acm_dense_prepare(items.data(), items.size(), wins.data(), wins.size(), opts, &dense, &D) == ACMHIP_OK && D.tables.size() == 16);
	wins.push_back(window(2, 0, 8, 1001, 1000));            // c = 31: the 17th
	CHECK(acm_dense_prepare(items.data(), items.size(), wins.data(), wins.size(), opts, &dense, &D) == ACMHIP_ERR_ARG);
	wins.back() = window(15, 0, 8, 0, 0);                   // an exact one: the 17th
	CHECK(acm_dense_prepare(items.data(), items.size(), wins.data(), wins.size(), opts, &dense, &D) == ACMHIP_ERR_ARG);
	wins.back() = window(0, 0, 8, 9, 0);                    // half a speed
	CHECK(acm_dense_prepare(items.data(), items.size(), wins.data(), wins.size(), opts, &dense, &D) == ACMHIP_ERR_ARG);
	printf("ok\n");
	return 0;
}
