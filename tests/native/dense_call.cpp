// The device-free description of a dense-family call under AddressSanitizer + UBSan (tests/test_dense_call.py builds and runs this):
// g++ -fsanitize=address,undefined over acm_dense_call.h and the layouts it links; nothing here knows a device.  The jobs-arena map is
// held to a table worked out by hand - every number below is a literal, none is recomputed by the code under test -, pack() to the
// spans and bytes of one tiny call per shape inside a poisoned arena, and acm_dense_call() to its four refusals and their order.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "acm_dense_call.h"
#include "acm_hip.h"

using namespace acmbatch;

#define CHECK(c)                                                                \
	do {                                                                    \
		if (!(c)) {                                                     \
			fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
			return 1;                                               \
		}                                                               \
	} while (0)

static const size_t N = ACM_JOBS_NONE;          // a section the call does not have; as an expected offset: not looked at

// parser bytes, the four section sizes | the four offsets and the total.  With b the parser bytes rounded up to 64 (0 -> 0, 1 -> 64,
// 64 -> 64, 65 -> 128): a section begins at the end of the one before it, rounded up to 64; the total is the end of the last one
struct MapCase {
	size_t parser, dense_b, overlay_b, fir_b, feat_b, dense, overlay, fir, feat, total;
};
static const MapCase MAP[] = {
	// dense alone, 16 bytes: [b, b + 16)
	{ 0, 16, N, N, N, 0, N, N, N, 16 },           { 1, 16, N, N, N, 64, N, N, N, 80 },
	{ 64, 16, N, N, N, 64, N, N, N, 80 },         { 65, 16, N, N, N, 128, N, N, N, 144 },
	// overlay, 72 bytes behind them: b + 16 rounds up to b + 64
	{ 0, 16, 72, N, N, 0, 64, N, N, 136 },        { 1, 16, 72, N, N, 64, 128, N, N, 200 },
	{ 64, 16, 72, N, N, 64, 128, N, N, 200 },     { 65, 16, 72, N, N, 128, 192, N, N, 264 },
	// overlay with filter, 16 bytes: b + 136 rounds up to b + 192
	{ 0, 16, 72, 16, N, 0, 64, 192, N, 208 },     { 1, 16, 72, 16, N, 64, 128, 256, N, 272 },
	{ 64, 16, 72, 16, N, 64, 128, 256, N, 272 },  { 65, 16, 72, 16, N, 128, 192, 320, N, 336 },
	// features without filter, 72 bytes: the bank sits where the filter would
	{ 0, 16, 72, N, 72, 0, 64, N, 192, 264 },     { 1, 16, 72, N, 72, 64, 128, N, 256, 328 },
	{ 64, 16, 72, N, 72, 64, 128, N, 256, 328 },  { 65, 16, 72, N, 72, 128, 192, N, 320, 392 },
	// features with filter: b + 208 rounds up to b + 256
	{ 0, 16, 72, 16, 72, 0, 64, 192, 256, 328 },  { 1, 16, 72, 16, 72, 64, 128, 256, 320, 392 },
	{ 64, 16, 72, 16, 72, 64, 128, 256, 320, 392 }, { 65, 16, 72, 16, 72, 128, 192, 320, 384, 456 },
	// a filter section of 0 bytes is none: the rows of "features without filter" again
	{ 0, 16, 72, 0, 72, 0, 64, N, 192, 264 },     { 1, 16, 72, 0, 72, 64, 128, N, 256, 328 },
	{ 64, 16, 72, 0, 72, 64, 128, N, 256, 328 },  { 65, 16, 72, 0, 72, 128, 192, N, 320, 392 },
	// dense tables of 0 bytes: the total is where they would begin
	{ 0, 0, N, N, N, 0, N, N, N, 0 },             { 1, 0, N, N, N, 64, N, N, N, 64 },
	{ 64, 0, N, N, N, 64, N, N, N, 64 },          { 65, 0, N, N, N, 128, N, N, N, 128 },
	// 72 bytes of dense tables and an overlay section of 0 bytes: it has an offset, b + 72 rounded up, and the total ends there
	{ 0, 72, 0, N, N, 0, 128, N, N, 128 },        { 1, 72, 0, N, N, 64, 192, N, N, 192 },
	{ 64, 72, 0, N, N, 64, 192, N, N, 192 },      { 65, 72, 0, N, N, 128, 256, N, N, 256 },
	// 72, 16, 72 and a bank of 0 bytes: b + 144 -> b + 192, b + 264 -> b + 320
	{ 0, 72, 16, 72, 0, 0, 128, 192, 320, 320 },  { 1, 72, 16, 72, 0, 64, 192, 256, 384, 384 },
	{ 64, 72, 16, 72, 0, 64, 192, 256, 384, 384 }, { 65, 72, 16, 72, 0, 128, 256, 320, 448, 448 },
	// nothing but a bank of 16 bytes: three empty sections share its offset
	{ 0, 0, 0, 0, 16, 0, 0, N, 0, 16 },           { 1, 0, 0, 0, 16, 64, 64, N, 64, 80 },
	{ 64, 0, 0, 0, 16, 64, 64, N, 64, 80 },       { 65, 0, 0, 0, 16, 128, 128, N, 128, 144 },
};

static int check_map()
{
	int cases = 0;
	for (const MapCase &c : MAP) {
		const JobsMap m = acm_jobs_map(c.parser, c.dense_b, c.overlay_b, c.fir_b, c.feat_b);
		CHECK(m.dense == c.dense && m.total == c.total);
		CHECK(c.overlay == N || m.overlay == c.overlay);
		CHECK(c.fir == N || m.fir == c.fir);
		CHECK(c.feat == N || m.feat == c.feat);
		// the properties, on what came out: multiples of 64, in order, disjoint, each as long as its size, the total the last one's end
		const size_t off[4] = { m.dense, m.overlay, m.fir, m.feat };
		const size_t len[4] = { c.dense_b, c.overlay_b, c.fir_b ? c.fir_b : N, c.feat_b };
		size_t end = c.parser;
		for (int s = 0; s < 4; s++) {
			if (len[s] == N)
				continue;
			CHECK(off[s] % 64 == 0 && off[s] >= end && off[s] - end < 64);
			end = off[s] + len[s];
		}
		CHECK(m.total == end);
		cases++;
	}
	// where the dense tables begin does not depend on what follows them: DenseLayout::table_off is this value
	CHECK(acm_jobs_map(65, 0, N, 0, N).dense == 128 && acm_jobs_map(65, 4096, 72, 16, 72).dense == 128);
	printf("dense_call: %d map cases\n", cases);
	return 0;
}

static WindowItem item()
{
	WindowItem it;
	it.info.channels = 1;
	it.info.rate = 16000;
	it.info.rows = 16;
	it.info.cols = 32;
	it.info.total_values = 1u << 16;
	it.len = 1u << 16;
	it.ok = true;
	it.whole = 1u << 16;
	return it;
}

// what one tiny call is made of: 3 windows of one stream, 2 output rows - row 0 in SNR mode over sources 0 and 1, row 1 source 2 as it is -,
// one 3-tap response on window 0, a bank of n_fft 128, hop 64 and one band of one weight
struct Tiny {
	WindowItem it = item();
	std::vector<acm_batch_window> wins;
	acm_batch_opts opts{};
	acm_dense_opts dense{ 128, 1, 0, 0, 0 };
	std::vector<acm_overlay_row> rows = { { 0, 1, 0, 65536, 0, 0, 0, 0 }, { 2, ACM_OVERLAY_NONE, 4096, 0, 0, 0, 0, 0 } };
	std::vector<int16_t> h = { 3, -2, 1 };
	acm_fir_response resp{};
	std::vector<uint32_t> of = { 0, ACM_FIR_NONE, ACM_FIR_NONE };
	acm_fir_opts fir{};
	std::vector<int16_t> window = std::vector<int16_t>(128, 100), cs = std::vector<int16_t>(128, -7);
	uint16_t first = 5, count = 1, w = 32768;
	uint32_t off = 0;
	acm_feat_bank bank{};
	Tiny()
	{
		for (uint64_t k = 0; k < 3; k++) {
			acm_batch_window win{};
			win.item = 0;
			win.first_word = 1000 * k;
			win.max_words = 128 - 8 * k;
			wins.push_back(win);
		}
		opts.fmt = ACMHIP_FMT_S16LE;
		opts.d_pcm = reinterpret_cast<int16_t *>(0x1000);
		opts.d_pcm_words = 1u << 20;
		resp = acm_fir_response{ h.data(), 3, 1, 2, 0 };
		fir = acm_fir_opts{ &resp, 1, of.data(), 0 };
		bank = acm_feat_bank{ 128, 64, 1, 0, window.data(), cs.data(), &first, &count, &off, &w, 0 };
	}
	int build(const DenseAsk &ask, DenseCall *c, const char **why) { return acm_dense_call(&it, 1, wins.data(), wins.size(), opts, ask, c, why); }
};

// one shape through pack(): the spans it must return (offsets and sizes as literals), the bytes at them, and every byte outside them
// left as it was
struct Shape {
	const char *name;
	DenseKind kind;
	bool with_fir;
	size_t nspan;
	JobsSpan span[4];
	size_t total;
};
// parser bytes 65: the dense tables at 128, 3 records of 16 bytes.  The overlay's at 192: 2 records of 24 bytes and 2 marked rows of 4
// are 56 up, then an energy of 8 per source row and 2 results of 24: 128 bytes with 3 source rows (ends at 320), 136 with the 4 of a
// call that filters one window (ends at 328, the filter's tables at 384: a tap block of 128 bytes and a row of 24, ending at 536).  The
// bank's tables at 320, or at 576 behind the filter's: 256 + 256 + 16 + 16 + 16 + 16 bytes
static const Shape SHAPES[] = {
	{ "dense", DENSE_ROWS, false, 1, { { 128, 48 } }, 176 },
	{ "overlay", DENSE_OVERLAY, false, 2, { { 128, 48 }, { 192, 56 } }, 320 },
	{ "overlay_fir", DENSE_OVERLAY, true, 3, { { 128, 48 }, { 192, 56 }, { 384, 152 } }, 536 },
	{ "features", DENSE_FEATURES, false, 3, { { 128, 48 }, { 192, 56 }, { 320, 576 } }, 896 },
	{ "features_fir", DENSE_FEATURES, true, 4, { { 128, 48 }, { 192, 56 }, { 384, 152 }, { 576, 576 } }, 1152 },
};

static int check_pack()
{
	Tiny t;
	for (const Shape &s : SHAPES) {
		const DenseAsk ask{ s.kind, &t.dense, s.kind == DENSE_ROWS ? nullptr : t.rows.data(), s.kind == DENSE_ROWS ? 0 : t.rows.size(),
				    s.with_fir ? &t.fir : nullptr, s.kind == DENSE_FEATURES ? &t.bank : nullptr };
		DenseCall c;
		const char *why = nullptr;
		CHECK(t.build(ask, &c, &why) == ACMHIP_OK && !why);
		CHECK((c.overlay() != nullptr) == (s.kind != DENSE_ROWS) && (c.fir() != nullptr) == s.with_fir && (c.feat() != nullptr) == (s.kind == DENSE_FEATURES));
		c.place(65);
		CHECK(c.map.total == s.total);
		// what staging left: window 1 lost its samples
		std::vector<WindowSlot> slots(3);
		std::vector<acm_batch_window> final = t.wins;
		for (size_t k = 0; k < 3; k++) {
			slots[k].active = true;
			slots[k].words = t.wins[k].max_words;
			slots[k].dev_off = 128 * k;
			final[k].words = k == 1 ? 0 : slots[k].words;
		}
		std::vector<uint8_t> arena(c.map.total, 0xA5);
		const DensePacked p = c.pack(arena.data(), slots.data(), final.data());
		CHECK(p.gather.kernel == DENSE_PLAIN && p.gather.bytes == 48 && p.nspan == s.nspan);
		std::vector<uint8_t> covered(arena.size(), 0);
		for (size_t i = 0; i < p.nspan; i++) {
			CHECK(p.span[i].off == s.span[i].off && p.span[i].bytes == s.span[i].bytes && p.span[i].off + p.span[i].bytes <= arena.size());
			memset(covered.data() + p.span[i].off, 1, p.span[i].bytes);
		}
		for (size_t at = 0; at < arena.size(); at++)
			CHECK(covered[at] || arena[at] == 0xA5);
		// the bytes at the spans are what the layout objects hold
		AcmDenseRow rows[3];
		CHECK(!acm_dense_rows(c.D, slots.data(), final.data(), rows) && rows[0].count == 128 && rows[1].count == 0 && rows[2].src == 256);
		CHECK(!memcmp(arena.data() + 128, rows, 48));
		size_t i = 1;
		if (c.overlay()) {
			// (window 0, filtered, is named by its row behind the windows: 3)
			CHECK(c.O.rows.size() == 2 && c.O.marked.size() == 2 && c.O.marked[0] == (s.with_fir ? 3u : 0u) && c.O.marked[1] == 1u);
			CHECK(!memcmp(arena.data() + 192, c.O.rows.data(), 48) && !memcmp(arena.data() + 192 + 48, c.O.marked.data(), 8));
			i++;
		}
		if (c.fir()) {
			CHECK(c.F.taps.size() == 64 && c.F.rows.size() == 1 && c.F.rows[0].src == 0 && c.F.rows[0].dst == 3);
			CHECK(!memcmp(arena.data() + 384, c.F.taps.data(), 128) && !memcmp(arena.data() + 384 + 128, c.F.rows.data(), 24));
			i++;
		}
		if (c.feat()) {
			std::vector<uint8_t> bank(c.M.table_bytes(), 0x5A);
			c.M.pack(bank.data());
			CHECK(bank.size() == 576 && !memcmp(arena.data() + p.span[i].off, bank.data(), 576));
			i++;
		}
		CHECK(i == p.nspan);
		printf("dense_call: pack %s\n", s.name);
	}
	// a filter call none of whose windows is filtered is an overlay call: no filter section, the overlay's tables as without it
	Tiny idle;
	idle.of[0] = ACM_FIR_NONE;
	const DenseAsk ask{ DENSE_FEATURES, &idle.dense, idle.rows.data(), idle.rows.size(), &idle.fir, &idle.bank };
	DenseCall c;
	const char *why = nullptr;
	CHECK(idle.build(ask, &c, &why) == ACMHIP_OK && !c.fir() && c.O.nsrc == 3);
	c.place(65);
	CHECK(c.map.feat == 320 && c.map.total == 896);
	return 0;
}

static int check_refusals()
{
	static const char *const DENSE = "acm_batch_decode_windows_dense: a call the dense writer does not take (include/acm_hip.h)";
	static const char *const OVERLAY = "acm_batch_decode_windows_overlay: a row table the call does not take (include/acm_hip.h)";
	static const char *const FIR = "acm_batch_decode_windows_overlay_fir: responses the call does not take (include/acm_hip.h)";
	static const char *const FEAT = "acm_batch_decode_windows_features: a bank or a tensor the call does not take (include/acm_hip.h)";
	// what is wrong with the call (dense options, row table, responses, bank) -> the text of the first part that refuses
	struct { bool dense, rows, fir, bank; const char *text; } set[] = {
		{ true, false, false, false, DENSE }, { false, true, false, false, OVERLAY }, { false, false, true, false, FIR }, { false, false, false, true, FEAT },
		{ true, true, true, true, DENSE },    { false, true, true, true, OVERLAY },   { false, false, true, true, FIR },  { true, false, false, true, DENSE },
		{ false, true, false, true, OVERLAY },
	};
	for (const auto &s : set) {
		Tiny t;
		if (s.dense)
			t.dense.channels = 3;
		if (s.rows)
			t.rows[1].a = 3;                // a source the call does not have
		if (s.fir)
			t.fir.reserved = 1;
		const DenseAsk ask{ DENSE_FEATURES, &t.dense, t.rows.data(), t.rows.size(), &t.fir, s.bank ? nullptr : &t.bank };
		DenseCall c;
		const char *why = nullptr;
		CHECK(t.build(ask, &c, &why) == ACMHIP_ERR_ARG && why && !strcmp(why, s.text));
	}
	// the parts a call does not have are not asked: a dense call takes bad rows, responses and bank, an overlay call a missing bank
	Tiny t;
	t.rows[1].a = 3;
	t.fir.reserved = 1;
	DenseCall c;
	const char *why = nullptr;
	const DenseAsk plain{ DENSE_ROWS, &t.dense, t.rows.data(), t.rows.size(), &t.fir, nullptr };
	CHECK(t.build(plain, &c, &why) == ACMHIP_OK && !why && !c.overlay() && !c.fir() && !c.feat());
	t.rows[1].a = 2;
	t.fir.reserved = 0;
	const DenseAsk over{ DENSE_OVERLAY, &t.dense, t.rows.data(), t.rows.size(), &t.fir, nullptr };
	CHECK(t.build(over, &c, &why) == ACMHIP_OK && c.overlay() && c.fir() && !c.feat());
	// the room behind d_pcm: a dense call's rows (3 * 128), an overlay call's (2 * 128), a features call's features (2 rows of 1 frame)
	t.opts.d_pcm_words = 383;
	CHECK(t.build(plain, &c, &why) == ACMHIP_ERR_ARG && !strcmp(why, DENSE));
	CHECK(t.build(over, &c, &why) == ACMHIP_OK);
	t.opts.d_pcm_words = 255;
	CHECK(t.build(over, &c, &why) == ACMHIP_ERR_ARG && !strcmp(why, OVERLAY));
	const DenseAsk feat{ DENSE_FEATURES, &t.dense, t.rows.data(), t.rows.size(), nullptr, &t.bank };
	t.opts.d_pcm_words = 2;
	CHECK(t.build(feat, &c, &why) == ACMHIP_OK && c.M.out_words == 2);
	t.opts.d_pcm_words = 1;
	CHECK(t.build(feat, &c, &why) == ACMHIP_ERR_ARG && !strcmp(why, FEAT));
	printf("dense_call: refusals\n");
	return 0;
}

int main()
{
	if (check_map() || check_pack() || check_refusals())
		return 1;
	printf("ok\n");
	return 0;
}
