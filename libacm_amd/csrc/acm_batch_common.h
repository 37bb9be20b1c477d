/*
 * acm_batch_common.h - what the batch front ends (acm_batch.cpp: whole files; acm_batch_windows.cpp: windows through a block index)
 * share: the worker pool, the arena arithmetic, the delivery rule of acm_read_loop().  Internal.
 */
#ifndef ACM_BATCH_COMMON_H
#define ACM_BATCH_COMMON_H

#include <sched.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "acm_hip.h"

namespace acmbatch {

using clk = std::chrono::steady_clock;
inline double secs(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }

/* How many words a caller looping over acm_read_loop() (acmtool.c:274-291)
 * gets out of `blocks` decodable blocks: blocks are drained whole except where
 * the per-call rounding to a multiple of `channels` (decode.c:856-857) or the
 * total_values cut (decode.c:853-854) stops the stream for good. */
inline uint64_t deliverable_words(uint64_t total_values, uint64_t block_len, unsigned channels, uint64_t blocks)
{
	uint64_t pos = 0;
	for (uint64_t b = 0; b < blocks && pos < total_values; b++) {
		uint64_t take = std::min(block_len, total_values - pos);
		if (channels > 1)
			take -= take % channels;
		pos += take;
		if (take != block_len)
			break;
	}
	return pos;
}

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

/* A fixed set of worker threads that lives for one acm_batch_decode call.  run() is a blocking parallel-for
 * (the caller works too); start()/wait() leave the caller free to drive the device meanwhile. */
class Pool {
public:
	explicit Pool(int threads)
	{
		for (int t = 0; t < threads; t++)
			workers_.emplace_back([this]() { loop(); });
	}
	~Pool()
	{
		{
			std::lock_guard<std::mutex> g(m_);
			quit_ = true;
		}
		cv_.notify_all();
		for (auto &t : workers_)
			t.join();
	}
	void start(size_t n, std::function<void(size_t)> fn)
	{
		std::lock_guard<std::mutex> g(m_);
		fn_ = std::move(fn);
		n_ = n;
		next_.store(0);
		active_ = workers_.size();
		gen_++;
		cv_.notify_all();
	}
	void wait()
	{
		std::unique_lock<std::mutex> g(m_);
		done_.wait(g, [this]() { return active_ == 0; });
	}
	void run(size_t n, const std::function<void(size_t)> &fn)
	{
		if (workers_.empty() || n <= 1) {
			for (size_t i = 0; i < n; i++)
				fn(i);
			return;
		}
		start(n, fn);
		for (size_t i; (i = next_.fetch_add(1)) < n;)
			fn(i);
		wait();
	}

private:
	void loop()
	{
		uint64_t seen = 0;
		for (;;) {
			{
				std::unique_lock<std::mutex> g(m_);
				cv_.wait(g, [&]() { return quit_ || gen_ != seen; });
				if (quit_)
					return;
				seen = gen_;
			}
			for (size_t i; (i = next_.fetch_add(1)) < n_;)
				fn_(i);
			std::lock_guard<std::mutex> g(m_);
			if (--active_ == 0)
				done_.notify_all();
		}
	}
	std::vector<std::thread> workers_;
	std::mutex m_;
	std::condition_variable cv_, done_;
	std::function<void(size_t)> fn_;
	std::atomic<size_t> next_{ 0 };
	size_t n_ = 0, active_ = 0;
	uint64_t gen_ = 0;
	bool quit_ = false;
};

inline uint64_t round_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

/* Blocks a file can possibly hold: the header promises total_values, but arenas are sized by this - a block costs at
 * least its 20-bit header and a 5-bit filler code per column (decode.c:491-502, 586-589), and the reader appends one
 * virtual zero byte (decode.c:57-61).  A 19-byte file that claims 2^32-1 samples gets one block, not 8 GB. */
inline uint64_t blocks_possible(const acm_stage_info &info, size_t len)
{
	const uint64_t bl = (uint64_t)info.rows * info.cols;
	const uint64_t promised = ((uint64_t)info.total_values + bl - 1) / bl;
	const uint64_t bits = (len > info.header_bytes ? (uint64_t)(len - info.header_bytes) * 8 : 0) + 8;
	return std::min<uint64_t>(promised, bits / (20 + 5 * (uint64_t)info.cols) + 1);
}

} // namespace acmbatch

#endif
