/*
 * acm_batch_windows.cpp - windowed batch decode: random-access crops out of many files in one call (include/acm_hip.h).
 *
 * No counterpart in the reference (it seeks by re-parsing a stream from its first block, util.c:219-242, one stream at a time).
 * With the block index of a file (acm_index.cpp) a window costs what the window holds: only the blocks from two rows in front of
 * its first sample to its last one are bit-parsed, cross PCIe, are synthesised and stored.  Each window becomes a pseudo-stream over
 * those blocks - a stream descriptor whose row_begin is the row of the first sample - and one plan over int16 rows covers the call.
 *
 *   host parsing    pool: acm_stage_window per window -> pinned arena -> one upload -> plan -> launch
 *   device parsing  pool: the byte span of every window's blocks -> pinned arena -> one upload -> acm_parse_scan_blocks (a wavefront
 *                   per block, checked against the marks) + acm_parse_columns -> results back -> the host stages the windows the
 *                   device gave up on -> plan -> launch
 *
 * The call is a straight line, not acm_batch.cpp's pipeline: a batch of windows is small by construction.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "acm_batch_common.h"
#include "acm_device.h"
#include "acm_hip.h"
#include "acm_index.h"
#include "libacm.h"

namespace {

using namespace acmbatch;

struct Item {
	acm_stage_info info{};
	bool ok = false;                /* an ACM file with an index it can have */
	int32_t end_status = 0;         /* what a window that reaches the end of the stream reports */
	uint64_t whole = 0;             /* words acm_batch_decode delivers for it */
};

struct Win {
	bool active = false;            /* has samples to decode */
	bool on_device = false;         /* staged by the device parser */
	uint32_t b0 = 0, nb = 0;        /* blocks staged: [b0, b0 + nb) */
	uint32_t row_begin = 0;         /* row of the first sample, counted from block b0 */
	uint64_t lead = 0;              /* samples of that row in front of the first one wanted */
	uint64_t idx_off = 0, hdr_off = 0, col_off = 0;
	uint64_t span_lo = 0, span_len = 0, file_off = 0;       /* device parsing: bytes [span_lo, span_lo + span_len) of the file, and their place */
	std::vector<acmhip_patch> patches;
};

/* what a call holds behind the arena lock; its end is every return's cleanup */
struct WinRun {
	ArenaLock lock;
	hipStream_t st;
	acmhip_plan *plan = nullptr;
	hipEvent_t ev[6] = {};
	WinRun(acmhip_device *dev, hipStream_t st_) : lock(dev), st(st_) {}
	~WinRun()
	{
		(void)hipStreamSynchronize(st);
		drop_unit(plan, ev, 6);
	}
};

constexpr uint64_t ACM_WINDOWS_AUTO_BLOCKS = 256;       /* ACM_BATCH_PARSE_AUTO: device parsing from this many staged blocks per call on */

/* samples in front of the first one wanted + the samples wanted, given how many the stream has */
inline uint64_t window_words(uint64_t whole, uint64_t first, uint64_t max_words)
{
	return first >= whole ? 0 : std::min(max_words, whole - first);
}

} // namespace

extern "C" uint64_t acm_batch_window_pcm_words(const acm_batch_item *items, size_t n, const acm_batch_window *wins, size_t nwin, int force_chans)
{
	std::vector<acm_stage_info> info(n);
	std::vector<char> ok(n, 0);
	for (size_t i = 0; items && i < n; i++)
		ok[i] = acm_stage_probe(items[i].data, items[i].len, force_chans, &info[i]) == ACM_OK;
	uint64_t total = 0;
	for (size_t k = 0; wins && k < nwin; k++) {
		const acm_batch_window &w = wins[k];
		if (w.item >= n || !ok[w.item])
			continue;
		const acm_stage_info &f = info[w.item];
		const uint64_t most = std::min<uint64_t>(f.total_values, blocks_possible(f, items[w.item].len) * f.rows * f.cols);
		const uint64_t words = window_words(most, w.first_word, w.max_words);
		if (words)
			total += round_up(w.first_word % f.cols + words, 64);
	}
	return total;
}

/* the call without its wall clock: the caller reads that once everything held here is released */
static int decode_windows(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index, acm_batch_window *wins,
			  size_t nwin, const acm_batch_opts *opts_in, acm_window_timing &tm)
{
	if (!dev)
		return ACMHIP_ERR_NO_DEVICE;
	if ((n && (!items || !index)) || (nwin && !wins))
		return ACMHIP_ERR_ARG;
	acm_batch_opts opts{};
	if (opts_in)
		opts = *opts_in;
	if (opts.fmt > 3 || opts.parse > ACM_BATCH_PARSE_AUTO || opts.prestaged || (opts.flags & ACM_BATCH_STAGE_PACKED))
		return ACMHIP_ERR_ARG;
	const bool out_f32 = (opts.flags & ACM_BATCH_PCM_F32) != 0;
	if (out_f32 && (!opts.d_pcm || opts.fmt != ACMHIP_FMT_S16LE)) {
		acmhip_set_error_text("ACM_BATCH_PCM_F32: device-resident output (opts->d_pcm) and ACMHIP_FMT_S16LE");
		return ACMHIP_ERR_ARG;
	}
	const bool keep_on_device = opts.d_pcm != nullptr;
	const int threads_wanted = opts.threads > 0 ? opts.threads : default_threads();
	Pool pool((int)std::min<size_t>((size_t)threads_wanted, std::max<size_t>(1, std::max(n, nwin))));

	/* 1. headers, and whether every index is one its file can have - before anything derived from it is used */
	std::vector<Item> its(n);
	pool.run(n, [&](size_t i) {
		Item &it = its[i];
		const int rc = acm_stage_probe(items[i].data, items[i].len, opts.force_chans, &it.info);
		if (rc != ACM_OK) {
			it.end_status = rc;
			return;
		}
		const uint64_t bl = (uint64_t)it.info.rows * it.info.cols;
		const uint64_t promised = ((uint64_t)it.info.total_values + bl - 1) / bl;
		if (index[i].blocks > promised || !acmindex::index_plausible(it.info, items[i].len, index[i].marks, index[i].blocks)) {
			it.end_status = ACMHIP_ERR_ARG;
			return;
		}
		it.ok = true;
		it.end_status = index[i].end_status;
		it.whole = deliverable_words(it.info.total_values, bl, it.info.channels, index[i].blocks);
	});

	/* 2. the windows: block ranges and arena layout */
	std::vector<Win> ws(nwin);
	uint64_t idx_total = 0, hdr_total = 0, pcm_total = 0, cols_total = 0, files_total = 0, max_columns = 0;
	std::vector<size_t> act, dev_ids;
	for (size_t k = 0; k < nwin; k++) {
		acm_batch_window &w = wins[k];
		Win &s = ws[k];
		w.words = 0;
		w.dev_off = w.slot_off = pcm_total;
		w.slot_words = 0;
		if (w.item >= n) {
			w.status = ACMHIP_ERR_ARG;
			continue;
		}
		const Item &it = its[w.item];
		const uint64_t words = window_words(it.whole, w.first_word, w.max_words);
		w.status = words == w.max_words ? ACM_OK : it.end_status;
		if (!words)
			continue;
		const uint64_t cols = it.info.cols, rows = it.info.rows;
		const uint64_t first_row = w.first_word / cols, last_row = (w.first_word + words - 1) / cols;
		s.b0 = (uint32_t)((first_row > 2 ? first_row - 2 : 0) / rows);
		s.nb = (uint32_t)(last_row / rows + 1 - s.b0);
		s.row_begin = (uint32_t)(first_row - (uint64_t)s.b0 * rows);
		s.lead = w.first_word - first_row * cols;
		s.active = true;
		s.idx_off = idx_total;
		s.hdr_off = hdr_total;
		w.words = words;
		w.slot_words = round_up(s.lead + words, 64);
		w.dev_off = w.slot_off + s.lead;
		idx_total += round_up((uint64_t)s.nb * rows * cols, 64);
		hdr_total += s.nb;
		pcm_total += w.slot_words;
		tm.blocks_parsed += s.nb;
		act.push_back(k);
	}
	/* AUTO: the host pool below ACM_WINDOWS_AUTO_BLOCKS staged blocks, the device walk from there on (measured on an MI355X with 16 host
	 * threads, profiles/window_decode_notes.txt: the device path pays ~0.15 ms more per call - a second round trip for the walk's results -
	 * and ~1.3 us less per block) */
	const bool dev_parse = opts.parse == ACM_BATCH_PARSE_DEVICE || (opts.parse == ACM_BATCH_PARSE_AUTO && tm.blocks_parsed >= ACM_WINDOWS_AUTO_BLOCKS);
	for (size_t a = 0; dev_parse && a < act.size(); a++) {
		const size_t k = act[a];
		const acm_batch_window &w = wins[k];
		Win &s = ws[k];
		const Item &it = its[w.item];
		/* the bytes that hold the window's blocks, from a dword boundary of the file; offsets inside count from there */
		const acm_block_mark *mk = index[w.item].marks;
		s.span_lo = (mk[s.b0].bit >> 3) & ~3ull;
		const uint64_t end_bit = mk[s.b0 + s.nb].bit - 8 * s.span_lo;
		s.span_len = std::min<uint64_t>(items[w.item].len, (mk[s.b0 + s.nb].bit + 7) >> 3) - s.span_lo;
		if (acmk_parse_supported(it.info.level, it.info.rows, s.span_len, s.nb) && end_bit <= 8 * s.span_len) {
			s.on_device = true;
			s.file_off = files_total;
			s.col_off = cols_total;
			files_total += file_slot_bytes(s.span_len);
			cols_total += (uint64_t)s.nb * it.info.cols;
			max_columns = std::max(max_columns, (uint64_t)s.nb * it.info.cols);
			dev_ids.push_back(k);
		}
	}
	if (keep_on_device && opts.d_pcm_words < pcm_total)
		return ACMHIP_ERR_ARG;
	if (dev_ids.size() > 0xFFFFFFFFull || hdr_total > 0xFFFFFFFFull)
		return ACMHIP_ERR_ARG;

	const auto t_hdr = clk::now();
	hipStream_t st = (hipStream_t)acmhip_device_stream(dev);
	int16_t *h_idx = nullptr, *d_idx = nullptr, *d_pcm = nullptr, *h_pcm = nullptr;
	acmhip_blkhdr *h_hdr = nullptr, *d_hdr = nullptr;
	uint8_t *h_files = nullptr, *d_files = nullptr, *h_jobs = nullptr, *d_jobs = nullptr;
	uint32_t *d_colpos = nullptr;
	WinRun run(dev, st);
	hipEvent_t *const ev = run.ev;
	const size_t pcm_unit = out_f32 ? sizeof(float) : sizeof(int16_t);
	const size_t nd = dev_ids.size();
	uint64_t nbj = 0;
	for (size_t k : dev_ids)
		nbj += ws[k].nb;
	const size_t jobs_bytes = round_up(nd * sizeof(AcmParseJob), 64), bjobs_bytes = round_up(nbj * sizeof(AcmBlockJob), 64);
	const size_t res_bytes = nd * (sizeof(AcmParseResult) + sizeof(uint32_t));      /* results, then flags */
	const bool host_arena = nd < act.size();                                        /* some window is staged by the host from the start */
	if (!act.empty()) {
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_IDX, idx_total * sizeof(int16_t), (void **)&d_idx));
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_HDR, hdr_total * sizeof(acmhip_blkhdr), (void **)&d_hdr));
		if (host_arena)
			ACM_TRY(host_arenas(dev, idx_total, hdr_total, &h_idx, &h_hdr));
		if (keep_on_device) {
			d_pcm = static_cast<int16_t *>(opts.d_pcm);
		} else {
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_PCM, pcm_total * pcm_unit, (void **)&d_pcm));
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_PCM, pcm_total * pcm_unit, (void **)&h_pcm));
		}
		if (nd) {
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_FILES, files_total, (void **)&h_files));
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_FILES, files_total, (void **)&d_files));
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_COLPOS, cols_total * sizeof(uint32_t), (void **)&d_colpos));
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_JOBS, jobs_bytes + bjobs_bytes + res_bytes, (void **)&h_jobs));
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_JOBS, jobs_bytes + bjobs_bytes + res_bytes, (void **)&d_jobs));
		}
		ACM_TRY(make_events(ev, 6));
	}
	const auto t_alloc = clk::now();
	tm.alloc_s = secs(t_hdr, t_alloc);

	/* the host stager of one window; a window whose blocks are not what the index says delivers nothing */
	auto host_stage = [&](size_t k) {
		Win &s = ws[k];
		acm_batch_window &w = wins[k];
		const acm_batch_item &f = items[w.item];
		acm_stage_info info;
		s.patches.clear();
		const int r = acmindex::stage_window(f.data, f.len, opts.force_chans, index[w.item].marks, index[w.item].blocks, s.b0, s.nb,
						     h_idx + s.idx_off, h_hdr + s.hdr_off, &s.patches, &info);
		if (r != ACM_OK || info.blocks != s.nb) {
			w.status = r != ACM_OK ? r : info.end_status ? info.end_status : ACM_ERR_CORRUPT;
			w.words = 0;
			s.active = false;
		}
	};

	/* 3. bit parsing */
	bool timed_h2d = false;
	if (!act.empty() && !dev_parse) {
		pool.run(act.size(), [&](size_t a) { host_stage(act[a]); });
		tm.host_parsed = act.size();
		tm.stage_s = secs(t_alloc, clk::now());
		ACM_HIP_TRY(hipEventRecord(ev[0], st));
		ACM_HIP_TRY(hipMemcpyAsync(d_idx, h_idx, idx_total * sizeof(int16_t), hipMemcpyHostToDevice, st));
		ACM_HIP_TRY(hipMemcpyAsync(d_hdr, h_hdr, hdr_total * sizeof(acmhip_blkhdr), hipMemcpyHostToDevice, st));
		ACM_HIP_TRY(hipEventRecord(ev[1], st));
		timed_h2d = true;
		tm.h2d_bytes += idx_total * sizeof(int16_t) + hdr_total * sizeof(acmhip_blkhdr);
	} else if (!act.empty()) {
		AcmParseJob *jobs = reinterpret_cast<AcmParseJob *>(h_jobs);
		AcmBlockJob *bjobs = reinterpret_cast<AcmBlockJob *>(h_jobs + jobs_bytes);
		std::vector<uint64_t> bj_at(nd + 1, 0);
		for (size_t a = 0; a < nd; a++)
			bj_at[a + 1] = bj_at[a] + ws[dev_ids[a]].nb;
		pool.run(nd, [&](size_t a) {
			const size_t k = dev_ids[a];
			const Win &s = ws[k];
			const acm_batch_item &f = items[wins[k].item];
			const Item &it = its[wins[k].item];
			const acm_block_mark *mk = index[wins[k].item].marks + s.b0;
			copy_zero_tail(h_files + s.file_off, f.data + s.span_lo, s.span_len, file_slot_bytes(s.span_len));
			AcmParseJob j{};
			j.file_off = s.file_off;
			j.idx_off = s.idx_off;
			j.hdr_off = s.hdr_off;
			j.col_off = s.col_off;
			j.file_len = (uint32_t)s.span_len;      /* a walk can never leave its span */
			j.level = it.info.level;
			j.rows = it.info.rows;
			j.blocks = s.nb;
			j.range_unit = 1;
			jobs[a] = j;
			for (uint32_t b = 0; b < s.nb; b++)
				bjobs[bj_at[a] + b] = AcmBlockJob{ (uint32_t)a, b, (uint32_t)(mk[b].bit - 8 * s.span_lo), (uint32_t)(mk[b + 1].bit - 8 * s.span_lo),
								   mk[b].val << 4 | mk[b].pwr, 0 };
		});
		/* the windows the device parser does not take at all */
		if (host_arena) {
			std::vector<size_t> host_ids;
			for (size_t k : act)
				if (!ws[k].on_device)
					host_ids.push_back(k);
			pool.run(host_ids.size(), [&](size_t a) { host_stage(host_ids[a]); });
			tm.host_parsed += host_ids.size();
			for (size_t k : host_ids) {
				const Win &s = ws[k];
				const uint64_t words = (uint64_t)s.nb * its[wins[k].item].info.rows * its[wins[k].item].info.cols;
				ACM_HIP_TRY(hipMemcpyAsync(d_idx + s.idx_off, h_idx + s.idx_off, words * sizeof(int16_t), hipMemcpyHostToDevice, st));
				ACM_HIP_TRY(hipMemcpyAsync(d_hdr + s.hdr_off, h_hdr + s.hdr_off, s.nb * sizeof(acmhip_blkhdr), hipMemcpyHostToDevice, st));
				tm.h2d_bytes += words * sizeof(int16_t) + s.nb * sizeof(acmhip_blkhdr);
			}
		}
		if (nd) {
			AcmParseResult *d_res = reinterpret_cast<AcmParseResult *>(d_jobs + jobs_bytes + bjobs_bytes);
			uint32_t *d_flags = reinterpret_cast<uint32_t *>(d_res + nd);
			ACM_HIP_TRY(hipEventRecord(ev[0], st));
			ACM_HIP_TRY(hipMemcpyAsync(d_files, h_files, files_total, hipMemcpyHostToDevice, st));
			ACM_HIP_TRY(hipMemcpyAsync(d_jobs, h_jobs, jobs_bytes + bjobs_bytes, hipMemcpyHostToDevice, st));
			ACM_HIP_TRY(hipEventRecord(ev[1], st));
			timed_h2d = true;
			tm.h2d_bytes += files_total + jobs_bytes + bjobs_bytes;
			ACM_HIP_TRY(hipMemsetAsync(d_res, 0, res_bytes, st));
			const int e = acmk_launch_parse_blocks(reinterpret_cast<const AcmParseJob *>(d_jobs), (uint32_t)nd,
							       reinterpret_cast<const AcmBlockJob *>(d_jobs + jobs_bytes), (uint32_t)nbj, d_files, d_colpos, d_idx,
							       d_hdr, d_res, d_flags, max_columns, st);
			if (e != 0)
				return acmhip_report_hip(e, "acmk_launch_parse_blocks");
			ACM_HIP_TRY(hipMemcpyAsync(h_jobs + jobs_bytes + bjobs_bytes, d_res, res_bytes, hipMemcpyDeviceToHost, st));
			ACM_HIP_TRY(hipStreamSynchronize(st));
			const AcmParseResult *res = reinterpret_cast<const AcmParseResult *>(h_jobs + jobs_bytes + bjobs_bytes);
			const uint32_t *flags = reinterpret_cast<const uint32_t *>(res + nd);
			/* what the device is not sure about goes to the exact reader: H1, bad symbols, a block that is not what its marks say */
			std::vector<size_t> redo;
			for (size_t a = 0; a < nd; a++)
				if (!parse_clean(res[a], flags[a], ws[dev_ids[a]].nb))
					redo.push_back(dev_ids[a]);
			tm.device_parsed = nd - redo.size();
			if (!redo.empty()) {
				ACM_TRY(host_arenas(dev, idx_total, hdr_total, &h_idx, &h_hdr));
				pool.run(redo.size(), [&](size_t a) { host_stage(redo[a]); });
				tm.host_parsed += redo.size();
				for (size_t k : redo) {
					const Win &s = ws[k];
					if (!s.active)
						continue;
					const uint64_t words = (uint64_t)s.nb * its[wins[k].item].info.rows * its[wins[k].item].info.cols;
					ACM_HIP_TRY(hipMemcpyAsync(d_idx + s.idx_off, h_idx + s.idx_off, words * sizeof(int16_t), hipMemcpyHostToDevice, st));
					ACM_HIP_TRY(hipMemcpyAsync(d_hdr + s.hdr_off, h_hdr + s.hdr_off, s.nb * sizeof(acmhip_blkhdr), hipMemcpyHostToDevice, st));
					tm.h2d_bytes += words * sizeof(int16_t) + s.nb * sizeof(acmhip_blkhdr);
				}
			}
		}
		tm.stage_s = secs(t_alloc, clk::now());
	}

	/* 4. one plan over every window that has samples: a pseudo-stream over its blocks, emitting from the row of its first sample */
	PlanStreams ps;
	for (size_t k : act) {
		const Win &s = ws[k];
		if (!s.active)
			continue;
		const acm_stage_info &info = its[wins[k].item].info;
		ps.add(info, s.idx_off, s.hdr_off, wins[k].slot_off, s.nb * info.rows, s.row_begin, s.lead + wins[k].words, s.patches);
		tm.samples += wins[k].words;
	}
	if (!ps.descs.empty()) {
		ACM_TRY(acmhip_plan_create(dev, ps.descs.data(), ps.descs.size(), ps.patches.data(), ps.patches.size(), opts.plan_flags, &run.plan));
		ACM_HIP_TRY(hipEventRecord(ev[2], st));
		ACM_TRY(launch_plan(run.plan, out_f32, d_idx, d_hdr, d_pcm, opts.fmt));
		ACM_HIP_TRY(hipEventRecord(ev[3], st));
		if (!keep_on_device) {
			ACM_HIP_TRY(hipEventRecord(ev[4], st));
			ACM_HIP_TRY(hipMemcpyAsync(h_pcm, d_pcm, pcm_total * pcm_unit, hipMemcpyDeviceToHost, st));
			ACM_HIP_TRY(hipEventRecord(ev[5], st));
		}
		ACM_HIP_TRY(hipStreamSynchronize(st));
		float ms = 0;
		if (timed_h2d && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
			tm.h2d_s = ms * 1e-3;
		if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess)
			tm.kernel_s = ms * 1e-3;
		if (!keep_on_device && hipEventElapsedTime(&ms, ev[4], ev[5]) == hipSuccess)
			tm.d2h_s = ms * 1e-3;
		if (!keep_on_device)
			pool.run(act.size(), [&](size_t a) {
				const acm_batch_window &w = wins[act[a]];
				if (ws[act[a]].active && w.pcm && w.words)
					memcpy(w.pcm, h_pcm + w.dev_off, std::min<uint64_t>(w.words, w.pcm_cap) * sizeof(int16_t));
			});
	}
	return ACMHIP_OK;
}

extern "C" int acm_batch_decode_windows(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index,
					acm_batch_window *wins, size_t nwin, const acm_batch_opts *opts_in, acm_window_timing *timing)
{
	acm_window_timing tm{};
	const auto t0 = clk::now();
	ACM_TRY(decode_windows(dev, items, n, index, wins, nwin, opts_in, tm));
	tm.total_s = secs(t0, clk::now());
	if (timing)
		*timing = tm;
	return ACMHIP_OK;
}
