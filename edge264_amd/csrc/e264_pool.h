#ifndef E264_POOL_H
#define E264_POOL_H
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>
// e264_pool.h -- a few host threads for the per-packet work of a batch that arrives in ordinary host memory (validation of every
// macroblock record + the copy into page-locked staging memory: 0.18 ms per 1080p packet on one thread = 5 k frames/s,
// while PCIe carries 28 k).  No HIP call is ever made from these threads.  E264_HOST_THREADS overrides the count (0: none).
// One pool per device: the submitter threads of several GPUs (e264_multi --devices) do not queue behind each other.
namespace {
struct HostPool {
	std::vector<std::thread> th;
	std::mutex m;
	std::condition_variable cv, done_cv;
	const std::function<void(int)> *fn = nullptr;
	std::atomic<int> next{0};
	int n = 0, active = 0, limit = 0;
	uint64_t gen = 0;
	bool stop = false, started = false;
	void run() { for (int i; (i = next.fetch_add(1)) < n;) (*fn)(i); }
	void worker(int id)
	{
		uint64_t seen = 0;
		std::unique_lock<std::mutex> lk(m);
		for (;;) {
			cv.wait(lk, [&] { return stop || gen != seen; });
			if (stop) return;
			seen = gen;
			const bool mine = id < limit; // (a job may ask for fewer workers than the pool has)
			lk.unlock();
			if (mine) run();
			lk.lock();
			if (--active == 0) done_cv.notify_one();
		}
	}
	// max_workers: pool threads that take part beside the caller (0: all).  Items that only copy (a trusted batch's gather into the staging buffer) are bound by
	// memory, not by cores: one buffer per stream (what a front end leaves) 106 / 109 / 108 k frames/s with 8 / 12 / 15 workers, four too few (66.7 k on one box);
	// tools/pin_probe.py, profiles/r06_ablations.txt item 17
	void parallel_for(int count, const std::function<void(int)> &f, int max_workers = 0)
	{
		std::unique_lock<std::mutex> lk(m);
		if (!started) {
			started = true;
			const char *e = getenv("E264_HOST_THREADS");
			int want = e ? atoi(e) : (int)std::min(15u, std::thread::hardware_concurrency() / 2);
			for (int i = 0; i < want; i++) th.emplace_back([this, i] { worker(i); });
		}
		if (th.empty() || count < 4) { lk.unlock(); for (int i = 0; i < count; i++) f(i); return; }
		fn = &f; n = count; next = 0; active = (int)th.size(); gen++;
		limit = max_workers > 0 ? max_workers : (int)th.size();
		lk.unlock();
		cv.notify_all();
		run(); // the caller works too
		lk.lock();
		done_cv.wait(lk, [&] { return active == 0; });
	}
	~HostPool()
	{
		{ std::lock_guard<std::mutex> lk(m); stop = true; }
		cv.notify_all();
		for (auto &t : th) t.join();
	}
};
}
#endif
