/*
 * acm_batch_windows.cpp - windowed batch decode: random-access crops out of many files in one call (include/acm_hip.h).
 *
 * No counterpart in the reference (it seeks by re-parsing a stream from its first block, util.c:219-242, one stream at a time).
 * With the block index of a file (acm_index_file, acm_stage.cpp) a window costs what the window holds: only the blocks from two rows in front of
 * its first sample to its last one are bit-parsed, cross PCIe, are synthesised and stored.  Each window becomes a pseudo-stream over
 * those blocks - a stream descriptor whose row_begin is the row of the first sample - and one plan over int16 rows covers the call.
 *
 *   host parsing    pool: acm_stage_window per window -> pinned arena -> one upload -> plan -> launch
 *   device parsing  pool: the byte span of every window's blocks -> pinned arena -> one upload -> acm_parse_scan_blocks (a wavefront
 *                   per block, checked against the marks) + acm_parse_columns -> results back -> the host stages the windows the
 *                   device gave up on -> plan -> launch
 *
 * Which blocks, where everything sits and who parses is acm_window_layout.cpp's, decided before the device is touched; this file
 * drives the device over that layout.  The call is a straight line, not acm_batch.cpp's pipeline: a batch of windows is small by
 * construction.
 *
 * acm_batch_decode_windows_dense is the same run with another end: the windows are synthesised into the handle's own PCM arena, nothing
 * is read back, and one launch of acm_dense_rows (acm_dense.hip) lays them out as the rows of the caller's tensor.  What that call
 * accepts, which windows it turns away and the kernel's row table are acm_dense_layout.cpp's - also, in one function
 * (acm_dense_tables), which kernel takes the launch: acm_dense_mixed's (acm_dense_mix.hip) where, with ACM_DENSE_MIX, a row of the
 * table converts between mono and stereo; acm_dense_resample's or acm_dense_speed's where, with ACM_DENSE_RESAMPLE and
 * ACM_DENSE_SPEED, a row is filtered to the batch's sample rate: then a second table and the ratios' taps travel with the first.
 *
 * acm_batch_decode_windows_overlay is the dense run with its gather launch aimed at the handle's source arena instead of the caller's
 * tensor, and two launches of acm_dense_overlay.hip behind it that make the caller's rows from those: which source rows get an
 * energy and where the tables sit is acm_overlay_layout.cpp's.
 *
 * acm_batch_decode_windows_overlay_fir is that run with one launch of acm_dense_fir.hip between the gather launch and the energy
 * launch: the windows acm_fir_layout.cpp lists are filtered into rows behind the source rows, and the overlay's tables name those.
 *
 * acm_batch_decode_windows_features is that run with its combine launch aimed at the handle's feature arena, int16, and two launches
 * of acm_dense_feat.hip behind it that make the caller's float32 features from those rows: the bank's check, its tables as they are
 * uploaded and the arena's layout are acm_feat_layout.cpp's.
 *
 * Which of these a call is, the layouts of its parts, where their tables sit in the H_JOBS / D_JOBS arenas and the bytes that go up
 * are acm_dense_call.h's (DenseCall): the five entry points say what was asked (DenseAsk), one decode_windows_dense builds the call,
 * and the driver reads offsets off its map and uploads the spans it packs.  What stays here is the device: arenas, copies, events
 * and the launchers - the switch over the gather kernels is the one place that knows them.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <optional>
#include <vector>

#include "acm_batch_common.h"
#include "acm_dense_call.h"
#include "acm_device.h"
#include "acm_hip.h"
#include "acm_stage.h"
#include "acm_window_layout.h"
#include "libacm.h"

namespace {

using namespace acmbatch;

/* One acm_batch_decode_windows call behind the arena lock: the device-side state over a WindowLayout it only reads.  The stages are
 * called once each, in the order of decode_windows; a stage that fails returns its code and the destructor is every return's cleanup */
class WinRun {
public:
	WinRun(acmhip_device *dev_, const acm_batch_item *items_, acm_batch_window *wins_, const acm_batch_opts &opts_,
	       const std::vector<WindowItem> &its_, const WindowLayout &L_, Pool &pool_, acm_window_timing &tm_, const DenseCall *call_, void *dense_out_,
	       acm_overlay_row *overlay_rows_)
		: lock(dev_), dev(dev_), items(items_), wins(wins_), opts(opts_), its(its_), L(L_), pool(pool_), tm(tm_), call(call_), dense_out(dense_out_),
		  overlay_rows(overlay_rows_), st((hipStream_t)acmhip_device_stream(dev_)), out_f32((opts_.flags & ACM_BATCH_PCM_F32) != 0),
		  keep_on_device(opts_.d_pcm != nullptr), pcm_unit(out_f32 ? sizeof(float) : sizeof(int16_t)), live(L_.slots.size())
	{
		for (size_t k : L.act)
			live[k].active = true;
	}
	~WinRun()
	{
		(void)hipStreamSynchronize(st);
		drop_unit(plan, ev, 6);
	}
	int fetch_arenas(clk::time_point t_hdr);        /* t_hdr: the layout was done, the wait for the arenas began */
	int parse_on_host();
	int parse_on_device();
	int synthesise_and_deliver();
	int synthesise_and_gather();

private:
	/* what a call changes about a window: the host stager rejects it, or finds H1 patches */
	struct Live {
		bool active = false;
		std::vector<acmhip_patch> patches;
	};
	const acm_stage_info &info_of(size_t k) const { return its[wins[k].item].info; }
	void stage_one(size_t k);
	void stage_on_host(const std::vector<size_t> &ids);
	int upload_slices(const std::vector<size_t> &ids);
	void collect(PlanStreams &ps);
	int launch_gather(const DenseLaunch &gather);
	int combine_rows();
	int make_features();
	void read_timers(bool d2h);

	ArenaLock lock;
	acmhip_device *const dev;
	const acm_batch_item *const items;
	acm_batch_window *const wins;
	const acm_batch_opts &opts;
	const std::vector<WindowItem> &its;
	const WindowLayout &L;
	Pool &pool;
	acm_window_timing &tm;
	const DenseCall *const call;            /* a call of the dense family (then opts are its inner ones: int16 rows, no caller memory), else null */
	void *const dense_out;                  /* ... its output tensor */
	acm_overlay_row *const overlay_rows;    /* ... and the caller's row table, for what comes back of an overlay call */
	const hipStream_t st;
	const bool out_f32, keep_on_device;
	const size_t pcm_unit;
	std::vector<Live> live;
	acmhip_plan *plan = nullptr;
	hipEvent_t ev[6] = {};
	bool timed_h2d = false;
	clk::time_point t_alloc;
	int16_t *h_idx = nullptr, *d_idx = nullptr, *d_pcm = nullptr, *h_pcm = nullptr;
	acmhip_blkhdr *h_hdr = nullptr, *d_hdr = nullptr;
	uint8_t *h_files = nullptr, *d_files = nullptr, *h_jobs = nullptr, *d_jobs = nullptr;
	uint32_t *d_colpos = nullptr;
	int16_t *d_src = nullptr;               /* the source rows of an overlay call */
	uint8_t *d_feat = nullptr;              /* the output rows of a features call, and the DFT's operand behind them */
};

/* Arenas (they live in the device handle and are reused by the next call) and events.  Needs nothing but the layout */
int WinRun::fetch_arenas(clk::time_point t_hdr)
{
	if (!L.act.empty()) {
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_IDX, L.idx_total * sizeof(int16_t), (void **)&d_idx));
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_HDR, L.hdr_total * sizeof(acmhip_blkhdr), (void **)&d_hdr));
		if (!L.host_ids.empty())                /* some window is staged by the host from the start */
			ACM_TRY(host_arenas(dev, L.idx_total, L.hdr_total, &h_idx, &h_hdr));
		if (keep_on_device) {
			d_pcm = static_cast<int16_t *>(opts.d_pcm);
		} else if (!call) {
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_PCM, L.pcm_total * pcm_unit, (void **)&d_pcm));
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_PCM, L.pcm_total * pcm_unit, (void **)&h_pcm));
		}
		if (!L.dev_ids.empty()) {
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_FILES, L.files_total, (void **)&h_files));
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_FILES, L.files_total, (void **)&d_files));
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_COLPOS, L.cols_total * sizeof(uint32_t), (void **)&d_colpos));
		}
	}
	if (call)               /* the intermediate PCM; a call without a window to decode still writes every row */
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_PCM, call->D.pcm_arena_words(L.pcm_total) * sizeof(int16_t), (void **)&d_pcm));
	if (call && call->overlay())
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_SRC, call->O.src_arena_words() * sizeof(int16_t), (void **)&d_src));
	if (call && call->feat())
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_FEAT, call->M.arena_bytes(), (void **)&d_feat));
	if (call || !L.dev_ids.empty()) {
		const size_t jobs_bytes = call ? call->map.total : L.job_arena_bytes();
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_JOBS, jobs_bytes, (void **)&h_jobs));
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_JOBS, jobs_bytes, (void **)&d_jobs));
	}
	if (call || !L.act.empty())
		ACM_TRY(make_events(ev, 6));
	t_alloc = clk::now();
	tm.alloc_s = secs(t_hdr, t_alloc);
	return ACMHIP_OK;
}

/* the host stager of one window; a window whose blocks are not what the index says delivers nothing */
void WinRun::stage_one(size_t k)
{
	const WindowSlot &s = L.slots[k];
	acm_batch_window &w = wins[k];
	const acm_batch_item &f = items[w.item];
	const WindowItem &it = its[w.item];
	acm_stage_info info;
	live[k].patches.clear();
	const int r = acmstage::stage_window(f.data, f.len, opts.force_chans, it.marks, it.blocks, s.b0, s.nb,
					     h_idx + s.idx_off, h_hdr + s.hdr_off, &live[k].patches, &info);
	if (r != ACM_OK || info.blocks != s.nb) {
		w.status = r != ACM_OK ? r : info.end_status ? info.end_status : ACM_ERR_CORRUPT;
		w.words = 0;
		live[k].active = false;
	}
}

void WinRun::stage_on_host(const std::vector<size_t> &ids)
{
	pool.run(ids.size(), [&](size_t a) { stage_one(ids[a]); });
	tm.host_parsed += ids.size();
}

/* the rows and headers of host-staged windows among device-staged ones, window by window; one the stager rejected has none */
int WinRun::upload_slices(const std::vector<size_t> &ids)
{
	for (size_t k : ids) {
		const WindowSlot &s = L.slots[k];
		if (!live[k].active)
			continue;
		const uint64_t words = window_rows_words(info_of(k), s.nb);
		ACM_HIP_TRY(hipMemcpyAsync(d_idx + s.idx_off, h_idx + s.idx_off, words * sizeof(int16_t), hipMemcpyHostToDevice, st));
		ACM_HIP_TRY(hipMemcpyAsync(d_hdr + s.hdr_off, h_hdr + s.hdr_off, s.nb * sizeof(acmhip_blkhdr), hipMemcpyHostToDevice, st));
		tm.h2d_bytes += words * sizeof(int16_t) + s.nb * sizeof(acmhip_blkhdr);
	}
	return ACMHIP_OK;
}

/* every window through the pool, the arenas up in one piece */
int WinRun::parse_on_host()
{
	stage_on_host(L.act);
	tm.stage_s = secs(t_alloc, clk::now());
	ACM_HIP_TRY(hipEventRecord(ev[0], st));
	ACM_HIP_TRY(hipMemcpyAsync(d_idx, h_idx, L.idx_total * sizeof(int16_t), hipMemcpyHostToDevice, st));
	ACM_HIP_TRY(hipMemcpyAsync(d_hdr, h_hdr, L.hdr_total * sizeof(acmhip_blkhdr), hipMemcpyHostToDevice, st));
	ACM_HIP_TRY(hipEventRecord(ev[1], st));
	timed_h2d = true;
	tm.h2d_bytes += L.idx_total * sizeof(int16_t) + L.hdr_total * sizeof(acmhip_blkhdr);
	return ACMHIP_OK;
}

/* the byte spans and the job tables up, the block walk and the column kernel, the verdicts back; the host stages the windows the
 * device parser does not take at all, and again the ones it is not sure about */
int WinRun::parse_on_device()
{
	const size_t nd = L.dev_ids.size();
	pool.run(nd, [&](size_t a) {
		const size_t k = L.dev_ids[a];
		const WindowSlot &s = L.slots[k];
		copy_zero_tail(h_files + s.file_off, items[wins[k].item].data + s.span_lo, s.span_len, file_slot_bytes(s.span_len));
	});
	if (!L.host_ids.empty()) {
		stage_on_host(L.host_ids);
		ACM_TRY(upload_slices(L.host_ids));
	}
	if (nd) {
		const size_t tables = L.res_off();
		memcpy(h_jobs, L.jobs.data(), nd * sizeof(AcmParseJob));
		memcpy(h_jobs + L.bjobs_off(), L.bjobs.data(), L.bjobs.size() * sizeof(AcmBlockJob));
		AcmParseResult *d_res = reinterpret_cast<AcmParseResult *>(d_jobs + tables);
		uint32_t *d_flags = reinterpret_cast<uint32_t *>(d_res + nd);
		ACM_HIP_TRY(hipEventRecord(ev[0], st));
		ACM_HIP_TRY(hipMemcpyAsync(d_files, h_files, L.files_total, hipMemcpyHostToDevice, st));
		ACM_HIP_TRY(hipMemcpyAsync(d_jobs, h_jobs, tables, hipMemcpyHostToDevice, st));
		ACM_HIP_TRY(hipEventRecord(ev[1], st));
		timed_h2d = true;
		tm.h2d_bytes += L.files_total + tables;
		ACM_HIP_TRY(hipMemsetAsync(d_res, 0, L.res_bytes, st));
		const acmhip_launch_caps caps = acmhip_device_launch_caps(dev);
		const int e = acmk_launch_parse_blocks(reinterpret_cast<const AcmParseJob *>(d_jobs), (uint32_t)nd,
						       reinterpret_cast<const AcmBlockJob *>(d_jobs + L.bjobs_off()), (uint32_t)L.bjobs.size(), d_files,
						       d_colpos, d_idx, d_hdr, d_res, d_flags, L.max_columns, caps.parse_slice, caps.parse_grid_x, st);
		if (e != 0)
			return acmhip_report_hip(e, "acmk_launch_parse_blocks");
		ACM_HIP_TRY(hipMemcpyAsync(h_jobs + tables, d_res, L.res_bytes, hipMemcpyDeviceToHost, st));
		ACM_HIP_TRY(hipStreamSynchronize(st));
		const AcmParseResult *res = reinterpret_cast<const AcmParseResult *>(h_jobs + tables);
		const uint32_t *flags = reinterpret_cast<const uint32_t *>(res + nd);
		/* what the device is not sure about goes to the exact reader: H1, bad symbols, a block that is not what its marks say */
		std::vector<size_t> redo;
		for (size_t a = 0; a < nd; a++)
			if (!parse_clean(res[a], flags[a], L.slots[L.dev_ids[a]].nb))
				redo.push_back(L.dev_ids[a]);
		tm.device_parsed = nd - redo.size();
		if (!redo.empty()) {
			ACM_TRY(host_arenas(dev, L.idx_total, L.hdr_total, &h_idx, &h_hdr));
			stage_on_host(redo);
			ACM_TRY(upload_slices(redo));
		}
	}
	tm.stage_s = secs(t_alloc, clk::now());
	return ACMHIP_OK;
}

/* every window that has samples as a stream of the call's plan: a pseudo-stream over its blocks, emitting from the row of its first sample */
void WinRun::collect(PlanStreams &ps)
{
	for (size_t k : L.act) {
		const WindowSlot &s = L.slots[k];
		if (!live[k].active)
			continue;
		ps.add(info_of(k), s.idx_off, s.hdr_off, s.slot_off, s.nb * info_of(k).rows, s.row_begin, s.lead + s.words, live[k].patches);
		tm.samples += s.words;
	}
}

/* one plan over those streams */
int WinRun::synthesise_and_deliver()
{
	PlanStreams ps;
	collect(ps);
	if (ps.descs.empty())
		return ACMHIP_OK;
	ACM_TRY(acmhip_plan_create(dev, ps.descs.data(), ps.descs.size(), ps.patches.data(), ps.patches.size(), opts.plan_flags, &plan));
	ACM_HIP_TRY(hipEventRecord(ev[2], st));
	ACM_TRY(launch_plan(plan, out_f32, d_idx, d_hdr, d_pcm, opts.fmt));
	ACM_HIP_TRY(hipEventRecord(ev[3], st));
	if (!keep_on_device) {
		ACM_HIP_TRY(hipEventRecord(ev[4], st));
		ACM_HIP_TRY(hipMemcpyAsync(h_pcm, d_pcm, L.pcm_total * pcm_unit, hipMemcpyDeviceToHost, st));
		ACM_HIP_TRY(hipEventRecord(ev[5], st));
	}
	ACM_HIP_TRY(hipStreamSynchronize(st));
	read_timers(!keep_on_device);
	if (!keep_on_device)
		pool.run(L.act.size(), [&](size_t a) {
			const acm_batch_window &w = wins[L.act[a]];
			if (live[L.act[a]].active && w.pcm && w.words)
				memcpy(w.pcm, h_pcm + w.dev_off, std::min<uint64_t>(w.words, w.pcm_cap) * sizeof(int16_t));
		});
	return ACMHIP_OK;
}

/* the events of a call whose stream is drained: the upload of the parse (where one was timed), the kernels, and the copy back where the
 * call made one */
void WinRun::read_timers(bool d2h)
{
	float ms = 0;
	if (timed_h2d && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
		tm.h2d_s = ms * 1e-3;
	if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess)
		tm.kernel_s = ms * 1e-3;
	if (d2h && hipEventElapsedTime(&ms, ev[4], ev[5]) == hipSuccess)
		tm.d2h_s = ms * 1e-3;
}

/* a dense call: the same plan into the handle's PCM arena, then the tables - what staging left of every window - up through the jobs
 * arena and one launch that writes every row of the caller's tensor, or the launches of an overlay or a features call behind it.
 * Nothing comes back but the timings and an overlay call's row results */
int WinRun::synthesise_and_gather()
{
	PlanStreams ps;
	collect(ps);
	if (!ps.descs.empty())
		ACM_TRY(acmhip_plan_create(dev, ps.descs.data(), ps.descs.size(), ps.patches.data(), ps.patches.size(), opts.plan_flags, &plan));
	const DensePacked packed = call->pack(h_jobs, L.slots.data(), wins);
	for (size_t i = 0; i < packed.nspan; i++) {
		const JobsSpan &up = packed.span[i];
		ACM_HIP_TRY(hipMemcpyAsync(d_jobs + up.off, h_jobs + up.off, up.bytes, hipMemcpyHostToDevice, st));
		tm.h2d_bytes += up.bytes;
	}
	ACM_HIP_TRY(hipEventRecord(ev[2], st));
	if (plan)
		ACM_TRY(launch_plan(plan, false, d_idx, d_hdr, d_pcm, ACMHIP_FMT_S16LE));
	ACM_TRY(launch_gather(packed.gather));
	if (call->overlay())
		ACM_TRY(combine_rows());
	if (call->feat())
		ACM_TRY(make_features());
	ACM_HIP_TRY(hipEventRecord(ev[3], st));
	const bool results = call->overlay() && !call->O.rows.empty();
	const size_t res_at = call->map.overlay + call->O.result_off();
	if (results) {
		ACM_HIP_TRY(hipEventRecord(ev[4], st));
		ACM_HIP_TRY(hipMemcpyAsync(h_jobs + res_at, d_jobs + res_at, call->O.result_bytes(), hipMemcpyDeviceToHost, st));
		ACM_HIP_TRY(hipEventRecord(ev[5], st));
	}
	ACM_HIP_TRY(hipStreamSynchronize(st));
	read_timers(results);
	if (results) {
		const AcmOverlayResult *res = reinterpret_cast<const AcmOverlayResult *>(h_jobs + res_at);
		for (size_t r = 0; r < call->O.rows.size(); r++)
			acm_overlay_report(res[r], &overlay_rows[r]);
	}
	return ACMHIP_OK;
}

/* the gather launch, by the kernel the tables were packed for.  An overlay call: the same launch writes the source rows, int16, and
 * the caller's tensor is combine_rows' */
int WinRun::launch_gather(const DenseLaunch &gather)
{
	const DenseLayout &D = call->D;
	const uint8_t *tab = d_jobs + call->map.dense;
	const AcmDenseRow *d_rows = reinterpret_cast<const AcmDenseRow *>(tab);
	const void *d_second = tab + D.resample_off();
	const int16_t *d_taps = reinterpret_cast<const int16_t *>(tab + D.taps_off());
	void *const rows_out = call->overlay() ? d_src : dense_out;
	const bool rows_f32 = call->overlay() ? false : D.f32;
	const acmhip_launch_caps caps = acmhip_device_launch_caps(dev);
	int e = 0;
	const char *name = nullptr;
	switch (gather.kernel) {
	case DENSE_SPEED:
		name = "acmk_launch_dense_speed";
		e = acmk_launch_dense_speed(d_pcm, d_rows, static_cast<const AcmSpeedRow *>(d_second), d_taps, L.slots.size(), rows_out, D.frames, D.channels,
					    D.planar, rows_f32, caps.dense_grid, st);
		break;
	case DENSE_RESAMPLE:
		name = "acmk_launch_dense_resample";
		e = acmk_launch_dense_resample(d_pcm, d_rows, static_cast<const AcmResampleRow *>(d_second), d_taps, L.slots.size(), rows_out, D.frames,
					       D.channels, D.planar, rows_f32, caps.dense_grid, st);
		break;
	case DENSE_MIXED:
		name = "acmk_launch_dense_mixed";
		e = acmk_launch_dense_mixed(d_pcm, d_rows, L.slots.size(), rows_out, D.frames, D.channels, D.planar, rows_f32, caps.dense_grid, st);
		break;
	case DENSE_PLAIN:
		name = "acmk_launch_dense_rows";
		e = acmk_launch_dense_rows(d_pcm, d_rows, L.slots.size(), rows_out, D.frames, D.channels, D.planar, rows_f32, caps.dense_grid, st);
		break;
	}
	return e != 0 ? acmhip_report_hip(e, name) : ACMHIP_OK;
}

/* an overlay call, behind the gather launch that wrote the source rows: the row table and the list of rows to sum went up with the
 * dense tables; the filtered rows are made first, where the call has any; the energies are zeroed and summed, and the combine launch
 * writes the caller's tensor and a result per row */
int WinRun::combine_rows()
{
	const DenseLayout *const dense = &call->D;
	const OverlayLayout *const overlay = &call->O;
	const FirLayout *const fir = call->fir();
	const size_t at = call->map.overlay;
	const acmhip_launch_caps caps = acmhip_device_launch_caps(dev);
	uint64_t *d_energy = reinterpret_cast<uint64_t *>(d_jobs + at + overlay->energy_off());
	if (fir) {
		const uint8_t *d_fir = d_jobs + call->map.fir;
		const int e = acmk_launch_dense_fir(d_src, reinterpret_cast<const AcmFirRow *>(d_fir + fir->rows_off()), fir->nfilt(),
						    reinterpret_cast<const uint32_t *>(d_fir), dense->frames, dense->channels, dense->planar, caps.dense_grid, st);
		if (e != 0)
			return acmhip_report_hip(e, "acmk_launch_dense_fir");
	}
	if (!overlay->marked.empty()) {
		ACM_HIP_TRY(hipMemsetAsync(d_energy, 0, overlay->energy_bytes(), st));
		const int e = acmk_launch_dense_energy(d_src, reinterpret_cast<const uint32_t *>(d_jobs + at + overlay->marked_off()), overlay->marked.size(),
						       overlay->row_words, d_energy, caps.dense_grid, st);
		if (e != 0)
			return acmhip_report_hip(e, "acmk_launch_dense_energy");
	}
	const int e = acmk_launch_dense_overlay(d_src, reinterpret_cast<const AcmOverlayRow *>(d_jobs + at), d_energy,
						reinterpret_cast<AcmOverlayResult *>(d_jobs + at + overlay->result_off()), overlay->rows.size(),
						call->feat() ? d_feat : dense_out, overlay->row_words, call->feat() ? false : dense->f32, caps.dense_grid, st);
	return e != 0 ? acmhip_report_hip(e, "acmk_launch_dense_overlay") : ACMHIP_OK;
}

/* a features call, behind the combine launch that wrote the int16 rows into the feature arena: the bank's tables went up with the
 * others; the DFT's operand is made of the cosines behind the rows, and the feature launch writes the caller's tensor */
int WinRun::make_features()
{
	const FeatLayout *const feat = &call->M;
	if (feat->out_words == 0)
		return ACMHIP_OK;
	const uint8_t *tab = d_jobs + call->map.feat;
	const acmhip_launch_caps caps = acmhip_device_launch_caps(dev);
	uint8_t *d_twiddle = d_feat + feat->twiddle_off();
	int e = acmk_launch_feat_twiddle(reinterpret_cast<const int16_t *>(tab + feat->cs_off()), feat->bank.n_fft, d_twiddle, st);
	if (e != 0)
		return acmhip_report_hip(e, "acmk_launch_feat_twiddle");
	AcmFeatDesc d{};
	d.n_fft = feat->bank.n_fft;
	d.hop = feat->bank.hop;
	d.n_mels = feat->bank.n_mels;
	d.flags = feat->bank.flags;
	d.window = reinterpret_cast<const int16_t *>(tab + feat->window_off());
	d.mel_first = reinterpret_cast<const uint16_t *>(tab + feat->first_off());
	d.mel_count = reinterpret_cast<const uint16_t *>(tab + feat->count_off());
	d.mel_off = reinterpret_cast<const uint32_t *>(tab + feat->off_off());
	d.mel_w = reinterpret_cast<const uint16_t *>(tab + feat->w_off());
	d.twiddle = d_twiddle;
	if (!feat->has_log) {
		e = acmk_launch_dense_feat(reinterpret_cast<const int16_t *>(d_feat), feat->nrows, feat->T, &d, static_cast<float *>(dense_out), caps.dense_grid, st);
		return e != 0 ? acmhip_report_hip(e, "acmk_launch_dense_feat") : ACMHIP_OK;
	}
	/* a logmel call: the scale goes with the launch, and the rows' maxima have their place behind the operand */
	d.log_flags = feat->log.flags;
	d.floor_q16 = feat->log.floor_q16;
	d.mul_q24 = feat->log.mul_q24;
	d.offset_q16 = feat->log.offset_q16;
	d.top_q16 = feat->log.top_q16;
	d.rowmax = feat->top() ? reinterpret_cast<int32_t *>(d_feat + feat->rowmax_off()) : nullptr;
	e = acmk_launch_dense_logmel(reinterpret_cast<const int16_t *>(d_feat), feat->nrows, feat->T, &d, static_cast<float *>(dense_out), caps.dense_grid, st);
	return e != 0 ? acmhip_report_hip(e, "acmk_launch_dense_logmel") : ACMHIP_OK;
}

/* headers, and whether every index is one its file can have - before anything derived from it is used */
std::vector<WindowItem> probe_items(Pool &pool, const acm_batch_item *items, size_t n, const acm_batch_index *index, int force_chans)
{
	std::vector<WindowItem> its(n);
	pool.run(n, [&](size_t i) {
		WindowItem &it = its[i];
		it.len = items[i].len;
		const int rc = acm_stage_probe(items[i].data, items[i].len, force_chans, &it.info);
		if (rc != ACM_OK) {
			it.end_status = rc;
			return;
		}
		const uint64_t bl = (uint64_t)it.info.rows * it.info.cols;
		const uint64_t promised = ((uint64_t)it.info.total_values + bl - 1) / bl;
		if (index[i].blocks > promised || !acmstage::index_plausible(it.info, items[i].len, index[i].marks, index[i].blocks)) {
			it.end_status = ACMHIP_ERR_ARG;
			return;
		}
		it.ok = true;
		it.end_status = index[i].end_status;
		it.whole = deliverable_words(it.info.total_values, bl, it.info.channels, index[i].blocks);
		it.marks = index[i].marks;
		it.blocks = index[i].blocks;
	});
	return its;
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
			total += window_slot_words(w.first_word % f.cols, words);
	}
	return total;
}

/* what every windowed call begins with: the arguments that must be there, the options with their defaults filled in, a pool sized for
 * the call's items and windows, and the items' headers */
struct Prelude {
	acm_batch_opts opts{};
	std::optional<Pool> pool;
	std::vector<WindowItem> its;
	int begin(const acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index, const acm_batch_window *wins, size_t nwin,
		  const acm_batch_opts *opts_in)
	{
		if (!dev)
			return ACMHIP_ERR_NO_DEVICE;
		if ((n && (!items || !index)) || (nwin && !wins))
			return ACMHIP_ERR_ARG;
		if (opts_in)
			opts = *opts_in;
		const int threads_wanted = opts.threads > 0 ? opts.threads : default_threads();
		pool.emplace((int)std::min<size_t>((size_t)threads_wanted, std::max<size_t>(1, std::max(n, nwin))));
		its = probe_items(*pool, items, n, index, opts.force_chans);
		return ACMHIP_OK;
	}
};

/* an entry point's wall clock around `call`, which fills in the rest: read once everything the call held is released.  A call that
 * fails leaves *timing alone */
template <typename F> int timed(acm_window_timing *timing, F &&call)
{
	acm_window_timing tm{};
	const auto t0 = clk::now();
	ACM_TRY(call(tm));
	tm.total_s = secs(t0, clk::now());
	if (timing)
		*timing = tm;
	return ACMHIP_OK;
}

/* the call without its wall clock */
static int decode_windows(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index, acm_batch_window *wins,
			  size_t nwin, const acm_batch_opts *opts_in, acm_window_timing &tm)
{
	Prelude pre;
	ACM_TRY(pre.begin(dev, items, n, index, wins, nwin, opts_in));
	const acm_batch_opts &opts = pre.opts;
	const std::vector<WindowItem> &its = pre.its;
	Pool &pool = *pre.pool;
	if (opts.fmt > 3 || opts.parse > ACM_BATCH_PARSE_AUTO || opts.prestaged || (opts.flags & ACM_BATCH_STAGE_PACKED))
		return ACMHIP_ERR_ARG;
	if ((opts.flags & ACM_BATCH_PCM_F32) && (!opts.d_pcm || opts.fmt != ACMHIP_FMT_S16LE)) {
		acmhip_set_error_text("ACM_BATCH_PCM_F32: device-resident output (opts->d_pcm) and ACMHIP_FMT_S16LE");
		return ACMHIP_ERR_ARG;
	}
	WindowLayout layout;
	const int laid = acm_window_layout(its.data(), n, wins, nwin, opts, &layout, &pool);
	for (size_t k = 0; k < nwin; k++) {             /* a refused call has told its windows their status and slots too */
		const WindowSlot &s = layout.slots[k];
		wins[k].status = s.status;
		wins[k].words = s.words;
		wins[k].slot_off = s.slot_off;
		wins[k].slot_words = s.slot_words;
		wins[k].dev_off = s.dev_off;
	}
	ACM_TRY(laid);
	tm.blocks_parsed = layout.blocks_parsed;

	const auto t_hdr = clk::now();
	WinRun run(dev, items, wins, opts, its, layout, pool, tm, nullptr, nullptr, nullptr);
	ACM_TRY(run.fetch_arenas(t_hdr));
	if (!layout.act.empty())
		ACM_TRY(layout.dev_parse ? run.parse_on_device() : run.parse_on_host());
	return run.synthesise_and_deliver();
}

/* a call of the dense family without its wall clock: what `ask` says of it, acm_dense_call.h describes */
static int decode_windows_dense(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index, acm_batch_window *wins,
				size_t nwin, const acm_batch_opts *opts_in, const DenseAsk &ask, acm_window_timing &tm)
{
	Prelude pre;
	ACM_TRY(pre.begin(dev, items, n, index, wins, nwin, opts_in));
	const std::vector<WindowItem> &its = pre.its;
	Pool &pool = *pre.pool;
	DenseCall call;
	const char *why = nullptr;
	if (acm_dense_call(its.data(), n, wins, nwin, pre.opts, ask, &call, &why) != ACMHIP_OK) {
		acmhip_set_error_text(why);
		return ACMHIP_ERR_ARG;
	}
	const DenseLayout &D = call.D;
	WindowLayout layout;
	ACM_TRY(acm_window_layout(its.data(), n, D.wins.data(), nwin, D.inner, &layout, &pool));
	for (size_t k = 0; k < nwin; k++) {
		acm_dense_report(D, layout.slots[k], k, &wins[k]);
		if (call.overlay())             /* nothing of d_pcm belongs to a window */
			wins[k].dev_off = wins[k].slot_off = wins[k].slot_words = 0;
	}
	tm.blocks_parsed = layout.blocks_parsed;
	if (!nwin)
		return ACMHIP_OK;
	call.place(layout.job_arena_bytes());

	const auto t_hdr = clk::now();
	WinRun run(dev, items, wins, D.inner, its, layout, pool, tm, &call, pre.opts.d_pcm, ask.rows);
	ACM_TRY(run.fetch_arenas(t_hdr));
	if (!layout.act.empty())
		ACM_TRY(layout.dev_parse ? run.parse_on_device() : run.parse_on_host());
	return run.synthesise_and_gather();
}

extern "C" int acm_batch_decode_windows_dense(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index,
					      acm_batch_window *wins, size_t nwin, const acm_batch_opts *opts_in, const acm_dense_opts *dense,
					      acm_window_timing *timing)
{
	const DenseAsk ask{ DENSE_ROWS, dense, nullptr, 0, nullptr, nullptr };
	return timed(timing, [&](acm_window_timing &tm) { return decode_windows_dense(dev, items, n, index, wins, nwin, opts_in, ask, tm); });
}

extern "C" int acm_batch_decode_windows_overlay(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index,
						acm_batch_window *wins, size_t nwin, const acm_batch_opts *opts_in, const acm_dense_opts *dense,
						acm_overlay_row *rows, size_t nrows, acm_window_timing *timing)
{
	const DenseAsk ask{ DENSE_OVERLAY, dense, rows, nrows, nullptr, nullptr };
	return timed(timing, [&](acm_window_timing &tm) { return decode_windows_dense(dev, items, n, index, wins, nwin, opts_in, ask, tm); });
}

extern "C" int acm_batch_decode_windows_overlay_fir(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index,
						    acm_batch_window *wins, size_t nwin, const acm_batch_opts *opts_in, const acm_dense_opts *dense,
						    const acm_fir_opts *fir, acm_overlay_row *rows, size_t nrows, acm_window_timing *timing)
{
	const DenseAsk ask{ DENSE_OVERLAY, dense, rows, nrows, fir, nullptr };
	return timed(timing, [&](acm_window_timing &tm) { return decode_windows_dense(dev, items, n, index, wins, nwin, opts_in, ask, tm); });
}

/* the two calls that end in features: `ask` is a features call's, with or without a scale */
static int decode_windows_features(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index, acm_batch_window *wins,
				   size_t nwin, const acm_batch_opts *opts_in, const DenseAsk &ask, acm_window_timing *timing)
{
	return timed(timing, [&](acm_window_timing &tm) { return decode_windows_dense(dev, items, n, index, wins, nwin, opts_in, ask, tm); });
}

extern "C" int acm_batch_decode_windows_features(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index,
						 acm_batch_window *wins, size_t nwin, const acm_batch_opts *opts_in, const acm_dense_opts *dense,
						 const acm_fir_opts *fir, const acm_feat_bank *bank, acm_overlay_row *rows, size_t nrows,
						 acm_window_timing *timing)
{
	const DenseAsk ask{ DENSE_FEATURES, dense, rows, nrows, fir, bank };
	return decode_windows_features(dev, items, n, index, wins, nwin, opts_in, ask, timing);
}

extern "C" int acm_batch_decode_windows_logmel(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index,
					       acm_batch_window *wins, size_t nwin, const acm_batch_opts *opts_in, const acm_dense_opts *dense,
					       const acm_fir_opts *fir, const acm_feat_bank *bank, const acm_feat_log *log, acm_overlay_row *rows, size_t nrows,
					       acm_window_timing *timing)
{
	if (!log) {
		acmhip_set_error_text("acm_batch_decode_windows_logmel: log is NULL (include/acm_hip.h)");
		return ACMHIP_ERR_ARG;
	}
	const DenseAsk ask{ DENSE_FEATURES, dense, rows, nrows, fir, bank, log };
	return decode_windows_features(dev, items, n, index, wins, nwin, opts_in, ask, timing);
}

extern "C" int acm_batch_decode_windows(acmhip_device *dev, const acm_batch_item *items, size_t n, const acm_batch_index *index,
					acm_batch_window *wins, size_t nwin, const acm_batch_opts *opts_in, acm_window_timing *timing)
{
	return timed(timing, [&](acm_window_timing &tm) { return decode_windows(dev, items, n, index, wins, nwin, opts_in, tm); });
}
