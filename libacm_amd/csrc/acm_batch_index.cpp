/*
 * acm_batch_index.cpp - the block index of many files in one call (include/acm_hip.h: acm_batch_index_files).
 *
 * No counterpart in the reference (it has no index: util.c:219-242 seeks by re-parsing).  acm_index_file runs the whole host parser
 * over a file to learn where its blocks start; the device only walks the stream (acm_parse.hip: acm_index_scan_wave) and writes
 * 16 bytes per block.  The batch travels in the groups acm_index_layout.cpp cut, through two halves of every arena:
 *
 *   pool: files of group k + 1 -> pinned half -> upload (aux stream 1)      |  overlap
 *   device stream: walk of group k -> marks and results back (pinned half)  |
 *   pool: the streams group k - 1 left dirty -> acm_index_file; its clean ones -> the callers' marks
 *
 * What the device is not sure about - a walk that was flagged or ended short, an end behind the file - is indexed again by the exact
 * reader; the result is acm_index_file's for every item, whoever did the work.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "acm_batch_common.h"
#include "acm_device.h"
#include "acm_hip.h"
#include "acm_index_layout.h"
#include "libacm.h"

namespace {

using namespace acmbatch;

enum { EV_UP0 = 0, EV_UP1, EV_K0, EV_K1, EV_D1, EV_PER_HALF };

/* what a call holds behind the arena lock; its end is every return's cleanup */
struct IndexRun {
	ArenaLock lock;
	hipStream_t st, up;
	hipEvent_t ev[2 * EV_PER_HALF] = {};
	IndexRun(acmhip_device *dev, hipStream_t st_, hipStream_t up_) : lock(dev), st(st_), up(up_) {}
	~IndexRun()
	{
		(void)hipStreamSynchronize(up);
		(void)hipStreamSynchronize(st);
		drop_unit(nullptr, ev, 2 * EV_PER_HALF);
	}
};

/* a stream of a group that has come back: its marks go out as they are, or the host reader takes it */
struct Task {
	size_t item;
	const acm_block_mark *marks;    /* null: acm_index_file */
	uint32_t blocks;
};

/* ACM_BATCH_PARSE_AUTO: the device when the batch is worth at least ACM_INDEX_AUTO_PER_THREAD x threads streams of its longest stream's
 * size - the shape of acm_batch_decode's rule, it is the same walk: a wavefront walks one stream at ~60 Msamples/s and a launch lasts as long as
 * its longest stream, a host thread indexes ~600 Msamples/s.  Measured on an MI355X with 16 host threads (profiles/index_build_notes.txt,
 * files of the corpus): this pool is ahead at 47 streams' worth (256 files: 15 against 48 ms) and at 105 (512 files: 30 against 52 ms), the
 * two meet at 196 (1024 files: 56 against 60 ms on the device) and the device is 1.7 x ahead at 731 (4000 files: 200 against 116 ms) */
constexpr uint64_t ACM_INDEX_AUTO_PER_THREAD = 12;

bool auto_device(const IndexItem *items, size_t n, const IndexLayout &L, int threads)
{
	uint64_t total = 0, longest = 0;
	for (size_t i = 0; i < n; i++) {
		const uint64_t words = L.slots[i].want_blocks * items[i].info.rows * items[i].info.cols;
		total += words;
		longest = std::max(longest, words);
	}
	return longest > 0 && total / longest >= ACM_INDEX_AUTO_PER_THREAD * (uint64_t)threads;
}

} // namespace

extern "C" uint64_t acm_batch_index_blocks(const acm_batch_item *items, size_t n, int force_chans, uint64_t *per_item)
{
	uint64_t total = 0;
	for (size_t i = 0; items && i < n; i++) {
		acm_stage_info info;
		const uint64_t b = acm_stage_probe(items[i].data, items[i].len, force_chans, &info) == ACM_OK ? blocks_possible(info, items[i].len) : 0;
		if (per_item)
			per_item[i] = b;
		total += b;
	}
	return total;
}

/* the call without its wall clock: the caller reads that once everything held here is released */
static int index_files(acmhip_device *dev, const acm_batch_item *items, size_t n, acm_batch_index_out *out, const acm_index_opts *opts_in,
		       acm_index_timing &tm)
{
	acm_index_opts opts{};
	opts.parse = ACM_BATCH_PARSE_AUTO;
	if (opts_in)
		opts = *opts_in;
	if ((n && (!items || !out)) || opts.parse > ACM_BATCH_PARSE_AUTO)
		return ACMHIP_ERR_ARG;
	if (opts.parse == ACM_BATCH_PARSE_DEVICE && !dev)
		return ACMHIP_ERR_NO_DEVICE;
	const int threads_wanted = opts.threads > 0 ? opts.threads : default_threads();
	Pool pool((int)std::min<size_t>((size_t)threads_wanted, std::max<size_t>(1, n)));

	auto host_index = [&](size_t i) {
		acm_stage_info info{};
		out[i].status = acm_index_file(items[i].data, items[i].len, opts.force_chans, out[i].marks, out[i].max_blocks, &info);
		out[i].blocks = info.blocks;
		out[i].end_status = info.end_status;
	};
	auto count_blocks = [&]() {
		for (size_t i = 0; i < n; i++)
			tm.blocks += out[i].blocks;
	};

	bool dev_walk = opts.parse == ACM_BATCH_PARSE_DEVICE;
	IndexLayout L;
	if (dev && opts.parse != ACM_BATCH_PARSE_HOST) {
		std::vector<IndexItem> its(n);
		pool.run(n, [&](size_t i) {
			IndexItem &it = its[i];
			it.ok = items[i].data && acm_stage_probe(items[i].data, items[i].len, opts.force_chans, &it.info) == ACM_OK;
			it.len = items[i].len;
			it.max_blocks = out[i].max_blocks;
			it.has_marks = out[i].marks != nullptr;
		});
		acm_index_layout(its.data(), n, opts.max_group_bytes, &L);
		if (opts.parse == ACM_BATCH_PARSE_AUTO)
			dev_walk = auto_device(its.data(), n, L, threads_wanted);
	}
	if (!dev_walk || L.dev_ids.empty()) {
		pool.run(n, host_index);
		tm.host_indexed = n;
		count_blocks();
		return ACMHIP_OK;
	}

	/* the arenas: two halves of each (one where the batch is a single group) */
	const size_t G = L.groups.size(), halves = std::min<size_t>(2, G);
	const uint64_t files_half = round_up(L.half_file_bytes, 256), marks_half = L.half_marks;
	const uint64_t jobs_half = round_up(L.half_jobs * sizeof(AcmParseJob), 256), res_half = round_up(L.half_jobs * sizeof(AcmParseResult), 256);
	void *st_v = acmhip_device_stream(dev), *up_v = nullptr;
	ACM_TRY(acmhip_aux_stream(dev, 1, &up_v));
	IndexRun run(dev, (hipStream_t)st_v, (hipStream_t)up_v);
	hipStream_t st = run.st, up = run.up;
	uint8_t *h_files = nullptr, *d_files = nullptr, *h_jobs = nullptr, *d_jobs = nullptr;
	acm_block_mark *h_marks = nullptr, *d_marks = nullptr;
	ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_FILES, halves * files_half, (void **)&h_files));
	ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_FILES, halves * files_half, (void **)&d_files));
	ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_JOBS, halves * (jobs_half + res_half), (void **)&h_jobs));
	ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_JOBS, halves * (jobs_half + res_half), (void **)&d_jobs));
	ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_MARKS, halves * marks_half * sizeof(acm_block_mark), (void **)&h_marks));
	ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_MARKS, halves * marks_half * sizeof(acm_block_mark), (void **)&d_marks));
	ACM_TRY(make_events(run.ev, halves * EV_PER_HALF));
	tm.groups = (uint32_t)G;
	tm.device_bytes = halves * (files_half + marks_half * sizeof(acm_block_mark) + jobs_half + res_half);

	/* group g's files and jobs into its pinned halves, and on their way up */
	auto stage = [&](size_t g) -> int {
		const IndexGroup &gr = L.groups[g];
		const size_t h = g & 1;
		hipEvent_t *ev = run.ev + h * EV_PER_HALF;
		const auto t0 = clk::now();
		uint8_t *hf = h_files + h * files_half;
		AcmParseJob *hj = reinterpret_cast<AcmParseJob *>(h_jobs + h * (jobs_half + res_half));
		pool.run(gr.k_last - gr.k_first, [&](size_t a) {
			const size_t k = gr.k_first + a, i = L.dev_ids[k];
			copy_zero_tail(hf + L.jobs[k].file_off, items[i].data, items[i].len, file_slot_bytes(items[i].len));
			hj[a] = L.jobs[k];
		});
		tm.stage_s += secs(t0, clk::now());
		const size_t njobs = gr.k_last - gr.k_first;
		ACM_HIP_TRY(hipEventRecord(ev[EV_UP0], up));
		ACM_HIP_TRY(hipMemcpyAsync(d_files + h * files_half, hf, gr.file_bytes, hipMemcpyHostToDevice, up));
		ACM_HIP_TRY(hipMemcpyAsync(d_jobs + h * (jobs_half + res_half), hj, njobs * sizeof(AcmParseJob), hipMemcpyHostToDevice, up));
		ACM_HIP_TRY(hipEventRecord(ev[EV_UP1], up));
		tm.h2d_bytes += gr.file_bytes + njobs * sizeof(AcmParseJob);
		return ACMHIP_OK;
	};
	/* its walk behind the upload, marks and results back behind the walk */
	auto launch = [&](size_t g) -> int {
		const IndexGroup &gr = L.groups[g];
		const size_t h = g & 1, njobs = gr.k_last - gr.k_first;
		hipEvent_t *ev = run.ev + h * EV_PER_HALF;
		uint8_t *dj = d_jobs + h * (jobs_half + res_half), *hj = h_jobs + h * (jobs_half + res_half);
		ACM_HIP_TRY(hipStreamWaitEvent(st, ev[EV_UP1], 0));
		ACM_HIP_TRY(hipEventRecord(ev[EV_K0], st));
		const int e = acmk_launch_index(reinterpret_cast<const AcmParseJob *>(dj), (uint32_t)njobs, d_files + h * files_half, d_marks + h * marks_half,
						reinterpret_cast<AcmParseResult *>(dj + jobs_half), st);
		if (e != 0)
			return acmhip_report_hip(e, "acmk_launch_index");
		ACM_HIP_TRY(hipEventRecord(ev[EV_K1], st));
		ACM_HIP_TRY(hipMemcpyAsync(h_marks + h * marks_half, d_marks + h * marks_half, gr.marks * sizeof(acm_block_mark), hipMemcpyDeviceToHost, st));
		ACM_HIP_TRY(hipMemcpyAsync(hj + jobs_half, dj + jobs_half, njobs * sizeof(AcmParseResult), hipMemcpyDeviceToHost, st));
		ACM_HIP_TRY(hipEventRecord(ev[EV_D1], st));
		return ACMHIP_OK;
	};
	/* wait for it and sort its streams: clean ones hand their marks out, the others go to the exact reader */
	auto finish = [&](size_t g, std::vector<Task> &tasks) -> int {
		const IndexGroup &gr = L.groups[g];
		const size_t h = g & 1;
		hipEvent_t *ev = run.ev + h * EV_PER_HALF;
		ACM_HIP_TRY(hipEventSynchronize(ev[EV_D1]));
		float ms = 0;
		if (hipEventElapsedTime(&ms, ev[EV_UP0], ev[EV_UP1]) == hipSuccess)
			tm.h2d_s += ms * 1e-3;
		if (hipEventElapsedTime(&ms, ev[EV_K0], ev[EV_K1]) == hipSuccess)
			tm.kernel_s += ms * 1e-3;
		if (hipEventElapsedTime(&ms, ev[EV_K1], ev[EV_D1]) == hipSuccess)
			tm.d2h_s += ms * 1e-3;
		const AcmParseResult *res = reinterpret_cast<const AcmParseResult *>(h_jobs + h * (jobs_half + res_half) + jobs_half);
		for (size_t k = gr.k_first; k < gr.k_last; k++) {
			const AcmParseJob &j = L.jobs[k];
			const AcmParseResult &r = res[k - gr.k_first];
			const acm_block_mark *mk = h_marks + h * marks_half + j.hdr_off;
			const bool clean = r.status == 0 && r.blocks_done == j.blocks && mk[j.blocks].bit <= 8ull * j.file_len;
			tasks.push_back(Task{ L.dev_ids[k], clean ? mk : nullptr, j.blocks });
			(clean ? tm.device_indexed : tm.host_indexed)++;
		}
		return ACMHIP_OK;
	};
	auto run_tasks = [&](std::vector<Task> &tasks) {
		pool.run(tasks.size(), [&](size_t a) {
			const Task &t = tasks[a];
			if (!t.marks) {
				host_index(t.item);
				return;
			}
			memcpy(out[t.item].marks, t.marks, ((size_t)t.blocks + 1) * sizeof(acm_block_mark));
			out[t.item].blocks = t.blocks;
			out[t.item].end_status = 0;
			out[t.item].status = ACM_OK;
		});
		tasks.clear();
	};

	/* the items the layout kept off the device travel with the first group's leftovers */
	std::vector<Task> pending, back;
	for (size_t i : L.host_ids)
		pending.push_back(Task{ i, nullptr, 0 });
	tm.host_indexed = L.host_ids.size();
	ACM_TRY(stage(0));
	for (size_t g = 0; g < G; g++) {
		ACM_TRY(launch(g));
		if (g + 1 < G)
			ACM_TRY(stage(g + 1));          /* (its halves are free: group g - 1 has been waited for) */
		run_tasks(pending);                     /* the host pool, while group g is on the device */
		ACM_TRY(finish(g, back));
		pending.swap(back);
	}
	run_tasks(pending);
	count_blocks();
	return ACMHIP_OK;
}

extern "C" int acm_batch_index_files(acmhip_device *dev, const acm_batch_item *items, size_t n, acm_batch_index_out *out,
				     const acm_index_opts *opts, acm_index_timing *timing)
{
	acm_index_timing tm{};
	const auto t0 = clk::now();
	ACM_TRY(index_files(dev, items, n, out, opts, tm));
	tm.total_s = secs(t0, clk::now());
	if (timing)
		*timing = tm;
	return ACMHIP_OK;
}
