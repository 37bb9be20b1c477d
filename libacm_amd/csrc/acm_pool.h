/*
 * acm_pool.h - the worker pool of a batch call.  Internal.  Knows no device: the front ends' drivers (acm_batch_common.h) and a
 * device-free layout that has a table worth filling in parallel (acm_window_layout.cpp) share it.
 */
#ifndef ACM_POOL_H
#define ACM_POOL_H

#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace acmbatch {

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

} // namespace acmbatch

#endif
