/*
 * acm_batch_common.h - what the batch front ends share.  Each is a device-free layout and a driver that only walks it:
 *   acm_batch.cpp          whole files                       over acm_batch_layout.cpp
 *   acm_batch_windows.cpp  windows through a block index     over acm_window_layout.cpp
 *   acm_batch_index.cpp    the block index of many files     over acm_index_layout.cpp
 * Here: the worker pool (acm_pool.h), the arena arithmetic and the delivery rule of acm_read_loop() (acm_batch_layout.h), and the
 * handful of steps the drivers take on the device - a call's hold on the arenas, its events, a plan's descriptors, the verdict on
 * the device parser's results, the file arena's zero tails, the launch.  Internal.
 */
#ifndef ACM_BATCH_COMMON_H
#define ACM_BATCH_COMMON_H

#include <hip/hip_runtime.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "acm_batch_layout.h"
#include "acm_device.h"
#include "acm_hip.h"
#include "acm_pool.h"

/* inside a function that returns an ACMHIP_* code: pass a failure on (its cleanup is the destructors') */
#define ACM_TRY(call) do { const int rc_ = (call); if (rc_ != ACMHIP_OK) return rc_; } while (0)
#define ACM_HIP_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return acmhip_report_hip((int)e_, #call); } while (0)

namespace acmbatch {

using clk = std::chrono::steady_clock;
inline double secs(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }

/* Default size of the parser pool.  Streams are independent and the parser is compute bound, so more threads
 * help up to the core count; past ~64 the returns vanish (and boxes with a cgroup CPU quota time-slice the
 * surplus), measured with profiles/e2e_probe.py. */
inline int default_threads()
{
	int n = (int)std::max(1u, std::thread::hardware_concurrency());
	cpu_set_t set;
	if (sched_getaffinity(0, sizeof(set), &set) == 0)
		n = std::min(n, std::max(1, CPU_COUNT(&set)));
	/* a cgroup-v2 CPU quota is invisible to the two calls above; threads beyond it only time-slice */
	if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
		long long quota = 0, period = 0;
		if (fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0)
			n = std::min<long long>(n, std::max<long long>(1, (quota + period - 1) / period));
		fclose(f);
	}
	return std::min(n, 64);
}

/* A call's hold on a device handle's arenas (they live in the handle and are reused by the next batch).  First member of a front end's
 * state object: whatever that object's destructor drains and destroys, the arenas are unlocked after it */
struct ArenaLock {
	acmhip_device *dev;
	explicit ArenaLock(acmhip_device *d) : dev(d) { acmhip_arena_lock(dev); }
	~ArenaLock() { acmhip_arena_unlock(dev); }
	ArenaLock(const ArenaLock &) = delete;
	ArenaLock &operator=(const ArenaLock &) = delete;
};

/* the events of one unit of work (a chunk, a range, a parse group, a call) ... */
inline int make_events(hipEvent_t *ev, size_t n)
{
	for (size_t k = 0; k < n; k++)
		ACM_HIP_TRY(hipEventCreateWithFlags(&ev[k], hipEventBlockingSync));
	return ACMHIP_OK;
}
/* ... and their end, with the unit's plan (either may be null).  The streams that use them are idle by then */
inline void drop_unit(acmhip_plan *plan, hipEvent_t *ev, size_t n)
{
	acmhip_plan_destroy(plan);
	for (size_t k = 0; k < n; k++)
		if (ev[k])
			(void)hipEventDestroy(ev[k]);
}

/* The host staging arenas, fetched when the first stream needs the exact host reader (with device parsing: perhaps never) */
inline int host_arenas(acmhip_device *dev, uint64_t idx_total, uint64_t hdr_total, int16_t **h_idx, acmhip_blkhdr **h_hdr)
{
	if (*h_idx)
		return ACMHIP_OK;
	ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_IDX, idx_total * sizeof(int16_t), (void **)h_idx));
	return acmhip_arena_get(dev, ACM_ARENA_H_HDR, hdr_total * sizeof(acmhip_blkhdr), (void **)h_hdr);
}

/* `have` bytes of a file into a slot of the pinned file arena, zeros behind them to the slot's end (a whole file's slot is
 * file_slot_bytes(): the device readers load whole dwords) */
inline void copy_zero_tail(uint8_t *dst, const uint8_t *src, uint64_t have, uint64_t slot)
{
	if (have)
		memcpy(dst, src, have);
	memset(dst + have, 0, slot - have);
}

/* did the device parser leave this job clean?  Anything else goes to the exact host reader: H1, bad symbols, data running out */
inline bool parse_clean(const AcmParseResult &res, uint32_t flags, uint64_t blocks)
{
	return res.status == 0 && res.blocks_done == blocks && flags == 0;
}

/* The streams of a plan as a front end collects them: descriptors, and every stream's H1 patches re-indexed to its descriptor */
struct PlanStreams {
	std::vector<acmhip_stream_desc> descs;
	std::vector<acmhip_patch> patches;
	/* rows [0, nrows) of a stream of `info`'s level and block height staged at idx_off / hdr_off; n_emit samples from row_begin on go to pcm_off */
	void add(const acm_stage_info &info, uint64_t idx_off, uint64_t hdr_off, uint64_t pcm_off, uint32_t nrows, uint32_t row_begin, uint64_t n_emit,
		 const std::vector<acmhip_patch> &stream_patches)
	{
		acmhip_stream_desc d{};
		d.idx_off = idx_off;
		d.hdr_off = hdr_off;
		d.pcm_off = pcm_off;
		d.level = info.level;
		d.rows = info.rows;
		d.nrows = nrows;
		d.row_begin = row_begin;
		d.n_emit = n_emit;
		for (acmhip_patch p : stream_patches) {
			p.stream = (uint32_t)descs.size();
			patches.push_back(p);
		}
		descs.push_back(d);
	}
};

/* every synthesis launch of a front end: int16 PCM in opts.fmt, or float32 (ACM_BATCH_PCM_F32: d_pcm holds floats) */
inline int launch_plan(acmhip_plan *plan, bool out_f32, const int16_t *d_idx, const acmhip_blkhdr *d_hdr, int16_t *d_pcm, unsigned fmt)
{
	return out_f32 ? acmhip_plan_launch_f32(plan, d_idx, d_hdr, reinterpret_cast<float *>(d_pcm)) : acmhip_plan_launch(plan, d_idx, d_hdr, d_pcm, fmt);
}

} // namespace acmbatch

#endif
