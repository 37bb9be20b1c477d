// Sanitizer harness for the block index and the window stager (libacm_amd/csrc/acm_stage.cpp): built with
// g++ -fsanitize=address,undefined, like fuzz_host.cpp; nothing it links knows a device.
//   - acm_index_file against acm_stage_file, on the files as they are and on a sweep of truncations;
//   - acm_stage_window against slices of acm_stage_file, every output buffer exactly as large as the call may fill;
//   - wrong indices (bits out of order, bits beyond the file, the index of another file, shifted marks, block_first beyond the index):
//     the call must refuse (ACMHIP_ERR_ARG), end with a status, or still produce the true slice - and never touch memory it should not.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "acm_hip.h"
#include "libacm.h"

/* (the tile geometries the stagers ask for are the library's own: this build links acm_kernel_geo.cpp, which needs no kernel) */

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)(rng >> 11); }

#define REQUIRE(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

struct Whole {
	acm_stage_info info{};
	std::vector<int16_t> idx;
	std::vector<acmhip_blkhdr> hdr;
	std::vector<acmhip_patch> patches;
	std::vector<acm_block_mark> marks;
	uint64_t bl = 0, need = 0;
	bool ok = false;
};

static bool same_info(const acm_stage_info &a, const acm_stage_info &b)
{
	return a.level == b.level && a.rows == b.rows && a.cols == b.cols && a.channels == b.channels && a.hdr_channels == b.hdr_channels &&
	       a.rate == b.rate && a.total_values == b.total_values && a.wavc == b.wavc && a.blocks == b.blocks && a.end_status == b.end_status &&
	       a.npatches == b.npatches && a.header_bytes == b.header_bytes;
}

/* acm_stage_file and acm_index_file of the same bytes must agree */
static Whole whole_file(const std::vector<uint8_t> &img, int force_chans)
{
	Whole w;
	acm_stage_info si;
	if (acm_stage_probe(img.data(), img.size(), force_chans, &si) != ACM_OK)
		return w;
	w.bl = (uint64_t)si.rows * si.cols;
	w.need = (si.total_values + w.bl - 1) / w.bl;
	if (w.need * w.bl >= (1u << 22))
		return w;
	w.idx.resize(w.need * w.bl);
	w.hdr.resize(w.need);
	REQUIRE(acm_stage_file(img.data(), img.size(), force_chans, w.idx.data(), w.hdr.data(), w.need, nullptr, 0, &w.info) == ACM_OK);
	w.patches.resize(w.info.npatches);
	REQUIRE(acm_stage_file(img.data(), img.size(), force_chans, w.idx.data(), w.hdr.data(), w.need, w.patches.data(), w.patches.size(), &w.info) == ACM_OK);
	w.marks.resize(w.need + 1);
	acm_stage_info ii;
	REQUIRE(acm_index_file(img.data(), img.size(), force_chans, w.marks.data(), w.need, &ii) == ACM_OK);
	REQUIRE(same_info(ii, w.info));
	w.marks.resize(w.info.blocks + 1);              /* exactly what the index holds: a read past it is a finding */
	for (uint32_t b = 0; b < w.info.blocks; b++) {
		REQUIRE(w.marks[b].val == w.hdr[b].val && w.marks[b].pwr == w.hdr[b].pwr);
		REQUIRE(w.marks[b].bit < w.marks[b + 1].bit);
	}
	w.ok = true;
	return w;
}

/* one window through marks `mk` (the file's own, or a wrong one); with the file's own index the slice must be exact */
static void window(const std::vector<uint8_t> &img, int force_chans, const Whole &w, const std::vector<acm_block_mark> &mk, size_t nidx, uint32_t first,
		   uint32_t count, bool own)
{
	std::vector<int16_t> idx((size_t)count * w.bl);
	std::vector<acmhip_blkhdr> hdr(count);
	std::vector<acmhip_patch> pt(w.patches.size());
	acm_stage_info si;
	const int rc = acm_stage_window(img.data(), img.size(), force_chans, mk.data(), nidx, first, count, idx.data(), hdr.data(), pt.data(), pt.size(), &si);
	if (rc != ACM_OK) {
		REQUIRE(!own || first > nidx);
		REQUIRE(rc == ACMHIP_ERR_ARG);
		return;
	}
	REQUIRE(si.blocks <= count);
	if (!own && (si.end_status != 0 || si.blocks == 0))
		return;
	/* staged blocks are the slice; so are the patches */
	const uint32_t avail = first < w.info.blocks ? w.info.blocks - first : 0;
	if (own) {
		REQUIRE(si.blocks == std::min(count, avail));
		REQUIRE(si.end_status == (count > avail ? w.info.end_status : 0));
	} else {
		REQUIRE(si.blocks <= avail);
	}
	REQUIRE(si.blocks == 0 || memcmp(idx.data(), w.idx.data() + (size_t)first * w.bl, (size_t)si.blocks * w.bl * sizeof(int16_t)) == 0);
	REQUIRE(si.blocks == 0 || memcmp(hdr.data(), w.hdr.data() + first, si.blocks * sizeof(acmhip_blkhdr)) == 0);
	if (!own)               /* (the (val, pwr) of marks in front of a window are taken on trust: nothing in the window can contradict them) */
		return;
	std::vector<acmhip_patch> want;
	for (const acmhip_patch &p : w.patches)
		if (p.sample >= (uint64_t)first * w.bl && p.sample < ((uint64_t)first + si.blocks) * w.bl)
			want.push_back(acmhip_patch{ p.sample - (uint64_t)first * w.bl, p.value, 0 });
	REQUIRE(si.npatches == want.size());
	for (size_t k = 0; k < want.size(); k++)
		REQUIRE(pt[k].sample == want[k].sample && pt[k].value == want[k].value);
}

static void own_windows(const std::vector<uint8_t> &img, int force_chans, const Whole &w)
{
	const uint32_t nb = w.info.blocks;
	window(img, force_chans, w, w.marks, nb, 0, nb + 1, true);
	window(img, force_chans, w, w.marks, nb, nb, 2, true);
	window(img, force_chans, w, w.marks, nb, nb + 1, 1, true);
	for (int k = 0; k < 6; k++) {
		const uint32_t first = rnd() % (nb + 1), count = rnd() % (nb + 2);
		window(img, force_chans, w, w.marks, nb, first, count, true);
	}
}

static void wrong_indices(const std::vector<uint8_t> &img, int force_chans, const Whole &w, const Whole *other)
{
	const uint32_t nb = w.info.blocks;
	if (nb < 2)
		return;
	for (int k = 0; k < 8; k++) {
		std::vector<acm_block_mark> mk = w.marks;
		const uint32_t at = rnd() % (nb + 1);
		switch (k % 4) {
		case 0: std::swap(mk[at % nb], mk[(at + 1) % nb]); break;                       /* out of order */
		case 1: mk[at].bit = 8ull * img.size() + 8 * (rnd() % 1000) + 9; break;         /* beyond the file */
		case 2: mk[at].bit += 1 + rnd() % 7; break;                                     /* a few bits off */
		default: mk[at].val ^= 1u << (rnd() % 16); break;                               /* another header */
		}
		window(img, force_chans, w, mk, nb, rnd() % nb, 1 + rnd() % nb, false);
	}
	if (other && other->ok && other->info.blocks >= 1) {
		/* the index of another file: as many of its marks as it has */
		const uint32_t nidx = other->info.blocks;
		window(img, force_chans, w, other->marks, nidx, rnd() % (nidx + 1), 1 + rnd() % (nidx + 1), false);
	}
}

int main(int argc, char **argv)
{
	if (argc < 3) {
		fprintf(stderr, "usage: fuzz_index CUTS file...\n");
		return 2;
	}
	const int cuts = atoi(argv[1]);
	std::vector<std::vector<uint8_t>> imgs;
	for (int a = 2; a < argc; a++) {
		FILE *f = fopen(argv[a], "rb");
		if (!f)
			continue;
		std::vector<uint8_t> img;
		uint8_t buf[65536];
		for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;)
			img.insert(img.end(), buf, buf + n);
		fclose(f);
		imgs.push_back(std::move(img));
	}
	size_t files = 0, windows_on = 0;
	Whole prev;
	for (const auto &img : imgs) {
		for (int fc = -1; fc <= 2; fc += 3) {
			const int force_chans = fc < 0 ? 0 : fc;
			const Whole w = whole_file(img, force_chans);
			if (!w.ok)
				continue;
			files++;
			own_windows(img, force_chans, w);
			wrong_indices(img, force_chans, w, prev.ok && prev.bl == w.bl ? &prev : nullptr);
			windows_on++;
			if (force_chans == 0)
				prev = w;
		}
		/* truncated anywhere: the index of the truncated file, and windows through it */
		for (int c = 0; c < cuts; c++) {
			std::vector<uint8_t> cut(img.begin(), img.begin() + rnd() % (img.size() + 1));
			cut.shrink_to_fit();
			const Whole w = whole_file(cut, 0);
			if (w.ok)
				own_windows(cut, 0, w);
		}
	}
	printf("index fuzz ok: %zu files, %zu with windows\n", files, windows_on);
	return 0;
}
