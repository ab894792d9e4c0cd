// e264_backend.hip -- C-ABI of the MI355X reconstruction back end (include/edge264_hip.h).
//
// Host side of the drop-in boundary: owns the device DPB of every decoder ("stream"), moves
// command packets to HBM with pinned async copies, launches the frame kernels on the compute
// lanes (HIP queues) of the device, and copies finished frames back on demand.  No torch types, no CPU
// fallback: if there is no gfx950 device every entry point fails with ENODEV.
//
// Queues of one device:
//   q[lane]  compute lanes.  A stream is bound to one lane (e264hip_stream_bind_lane, default 0); everything that touches
//            its DPB is ordered there.  Submissions of streams on different lanes run beside each other on the GPU.
//   qup      upload queue: the packet and job-table H2D copies of host batches.  A lane waits for ITS batch's copy event
//            only, so batch n+1 is in flight over PCIe while the kernels of batch n run (round 2: both shared one in-order
//            queue and a submission cost copy time + kernel time).
//   qc       download queue (edge264_get_frame's D2H beside the kernels).
// Nothing a single decoder does (frame_alloc / frame_free / flush / close / get_frame) waits for the device: each waits
// for that decoder's own last submission at most; memory it gives back is parked and recycled (hipFree would drain every
// queue of the device).
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "e264_kernels.h"
#include "e264_check.h" // the packet validation, API, e264_err / e264_fail
#include "e264_pool.h"

static int fail(int code, const char *what, hipError_t e = hipSuccess) { return e264_fail(code, what, e != hipSuccess ? hipGetErrorString(e) : nullptr); }
#define HIPCHK(call, code) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(code, #call, e_); } while (0)

// Build-time switches of this library, space separated; "" for the product build.  An E264_ABL_* / E264_PHASE_* entry means the
// kernels compute WRONG SAMPLES on purpose (timing ablations): such a library only opens a device with E264_ALLOW_ABLATION=1.
API const char *e264hip_build_flags(void) { return e264_kernel_build_flags(); }
static bool ablation_build_refused()
{
	const char *f = e264_kernel_build_flags();
	if (!strstr(f, "E264_ABL_") && !strstr(f, "E264_PHASE_")) return false;
	const char *a = getenv("E264_ALLOW_ABLATION");
	return !(a && a[0] == '1');
}
// events a host thread waits on: blocking, so that the waiter sleeps instead of spinning on a core the parser threads could use
#define E264_WAIT_EVENT (hipEventDisableTiming | hipEventBlockingSync)

struct E264Packet { E264Device *dev; uint8_t *d_bytes; E264PacketInfo info; }; // a packet that stays in HBM, as the kernels read it (version 4)

// A buffer that only grows (buf_grow): a page-locked block, a device block or both.  `cap` counts in its user's units and follows its user's rounding; the
// blocks' sizes are kept as they were asked for, because the recycler matches parked blocks by exact size.
struct GrowBuf {
	uint8_t *h = nullptr, *d = nullptr;
	size_t cap = 0, h_bytes = 0, d_bytes = 0;
};

#define E264_GATHER_WORKERS 12 // pool threads that gather a trusted batch into its staging buffer (copy only: see HostPool::parallel_for; E264_GATHER_THREADS overrides)
#define E264_JOB_RING 4 // batches in flight per device: one uploading, one in the kernels, one retiring
struct E264Device {
	int ordinal;
	enum { NQ = E264_MAX_LANES };
	hipStream_t q[NQ];         // compute lanes
	hipStream_t qup = nullptr; // upload queue
	hipStream_t qc = nullptr;  // download queue
	int waves;                 // option "waves": the deblocking kernel's form, a row of e264_forms (e264_plan.h)
	int intra_waves;           // option "intra_waves": waves per frame workgroup of the intra kernel (1 macroblock row each), a row of e264_forms
	std::atomic<int> lane_streams[NQ] = {}; // live streams bound to each lane (open, bind_lane, close): the lanes in use are those with one
	int n_cus;                 // compute units of the device
	int split_planes;          // option "split_planes" (default 1): the split-off pictures' intra pass with luma and chroma on two workgroups (e264_intra_planes_kernel)
	int split_intra;           // option "split_intra" (default 1): in a submission that mixes I pictures with others, their intra pass runs on q2 from the start (E264Plan.n_split)
	int side_queue;            // option "side_queue": parameter kernel on a second queue beside the macroblock-parallel kernel
	int upload_queue;          // option "upload_queue" (default 1): the H2D copies of host batches go through qup
	hipStream_t q2[NQ];        // one second queue per compute lane (+ its fork / join events): lanes must not share one (their split submissions would queue behind each other)
	hipEvent_t forked[NQ], joined[NQ];
	hipEvent_t lane_ev[NQ];    // e264hip_event_record: joins the other lanes into lane 0
	std::mutex lock;           // kernel launches + their timing marks + the submission event ring + launch_counts
	uint64_t launch_counts[E264_LC_COUNT] = {}; // pictures per kernel form (e264hip_launch_counts; slot E264_LC_N_CUS unused here)
	std::mutex batch_lock;     // host batches: job ring, staging
	hipEvent_t ev[16];
	// per-launch kernel timing
	bool ktiming;
	struct Marks { hipEvent_t e[5], a[2]; bool side; };
	std::vector<Marks> kev;
	size_t kev_used;
	// job tables of host-packet batches: a ring of pinned + device buffers, each with the event of its upload and of its kernels
	struct JobRing {
		GrowBuf jobs; // E264Job[cap], pinned + device
		hipEvent_t done = nullptr, up = nullptr; bool busy = false;
		// pageable batches: the packets of the WHOLE batch back to back in one page-locked buffer and one device buffer, so that a
		// batch crosses PCIe as ONE transfer (256 copies of 1 MB each reached 35 GB/s, and cost the submitting thread 257 driver calls)
		GrowBuf pkt;
		// wire packets of the batch (include/edge264_compact.h) are unfolded HERE, by e264_expand_kernel on the upload queue right behind the batch's copy --
		// beside the kernels of the batch before, whose streams read THEIR ring slot's buffer: nothing to order but what the ring already orders
		GrowBuf xp;
	} jring[E264_JOB_RING];
	int jring_next = 0;
	// Which submission wrote a slot last, and when it has retired: edge264_get_frame of ONE decoder must not wait for the
	// whole device (every later batch of every other decoder), only for the submission that produced its frame.
	uint64_t serial = 0;       // submissions so far (guarded by `lock`)
	enum { NEV = 1024 };       // (round 5: 64 wrapped at once when hundreds of decoders filled their slots -- every fill takes a serial -- and every wait fell back to the whole lane)
	hipEvent_t sub_ev[NEV] = {};
	uint64_t sub_serial[NEV] = {};
	int sub_lane[NEV] = {};
	std::atomic<uint64_t> lane_retired[NQ] = {}; // per lane: the highest serial anybody has SEEN retired (a lane runs in order: everything below has too)
	// Memory recycler.  hipFree / hipHostFree drain EVERY queue of the device, so what a decoder gives back (frame slots and
	// their host mirrors at an SPS change or edge264_free, parameter and staging buffers) is parked with the submission that
	// may still read it and handed to the next request of the same size once that submission has retired.  Parked memory is
	// released for real when the device closes (or when more than PARK_MAX blocks wait: the oldest retired ones go).
	struct Parked { void *p; size_t bytes; uint64_t serial; int lane; bool host; };
	enum { PARK_MAX = 4096 };
	std::vector<Parked> parked;
	std::mutex park_lock;
	HostPool pool;             // validation + staging copies of this device's host batches
	std::mutex pool_user;      // one batch at a time uses the pool
};

struct E264Stream {
	E264Device *dev;
	int lane;                             // compute lane of the device everything of this stream is ordered on
	uint8_t **d_table;                    // device array [E264_MAX_SLOTS] of slot pointers
	uint8_t *h_table[E264_MAX_SLOTS];     // same, host copy
	void *mirror[E264_MAX_SLOTS];         // pinned host mirrors
	size_t slot_bytes[E264_MAX_SLOTS];
	GrowBuf dbk;                          // per-stream scratch of the kernels: E264_SCRATCH_BYTES(dbk.cap macroblocks) (deblocking parameters + the intra bitmap)
	GrowBuf expand;                       // where e264_expand_kernel unfolds the wire packets (include/edge264_compact.h) of e264hip_frame_submit; empty until the first one (batches: the ring slot's buffer)
	// the slot table reaches the device from a small pinned ring (asynchronous: a pageable source would make hipMemcpyAsync
	// wait for the queue)
	enum { NTAB = 4 };
	uint8_t **tab_pin;                    // [NTAB][E264_MAX_SLOTS]
	hipEvent_t tab_ev[NTAB];
	bool tab_busy[NTAB];
	int tab_next;
	// packet staging ring (pinned host) + device copies
	struct Stage : GrowBuf { hipEvent_t done; bool busy; E264Job *d_job; } stage[4]; // (h: cap + 64 bytes, the job record rides at its tail)
	int stage_next;
	// Written by the decoder's own thread (fills, frees) AND by the thread that submits its batches (e264_multi: another one), hence
	// atomic and only ever raised: serials are handed out in queue order, so "the latest thing queued for this stream" is a maximum,
	// whichever thread's bookkeeping lands last.  (Round 3 kept a `loose` flag beside a plain serial: a submitter's late "no fill
	// pending" could erase a parser's "fill pending" and a freed slot went to another lane with the fill still queued.)
	std::atomic<uint64_t> slot_serial[E264_MAX_SLOTS]; // what wrote the slot last: a submission or a fill (0: nothing since it was allocated)
	std::atomic<uint64_t> last_serial;                 // the latest submission or fill of the stream
	hipEvent_t dl_done;                   // the stream's last download
};

static void raise_serial(std::atomic<uint64_t> &a, uint64_t v)
{
	uint64_t cur = a.load(std::memory_order_relaxed);
	while (cur < v && !a.compare_exchange_weak(cur, v, std::memory_order_relaxed)) {}
}
static void publish_serial(E264Stream *s, int slot, uint64_t serial) // submission or fill `serial` wrote the slot
{
	raise_serial(s->slot_serial[slot], serial);
	raise_serial(s->last_serial, serial);
}
static int set_device(E264Device *dev)
{
	HIPCHK(hipSetDevice(dev->ordinal), EIO);
	return 0;
}
static hipStream_t lane_of(const E264Stream *s) { return s->dev->q[s->lane]; }
static E264SlotView slots_of(const E264Stream *s) { return {s->h_table, s->slot_bytes}; }

// ---------------------------------------------------------------------------------------------------------------------
// submissions: retired? / wait
// ---------------------------------------------------------------------------------------------------------------------
// (dev->lock held) the next serial, its event recorded at the tail of the lane
static uint64_t next_serial(E264Device *dev, int lane)
{
	const uint64_t serial = ++dev->serial;
	const int idx = (int)(serial % E264Device::NEV);
	if (dev->sub_ev[idx] && hipEventRecord(dev->sub_ev[idx], dev->q[lane]) == hipSuccess) { dev->sub_serial[idx] = serial; dev->sub_lane[idx] = lane; }
	else dev->sub_serial[idx] = 0;
	return serial;
}
// A serial for work queued on a lane OUTSIDE a batch submission (a fill): same numbering, same event ring, so that whatever
// waits for "the stream's latest work" or parks memory behind it covers the fill too.
static uint64_t mark_lane(E264Device *dev, int lane)
{
	std::lock_guard<std::mutex> g(dev->lock);
	return next_serial(dev, lane);
}
static hipEvent_t serial_event(E264Device *dev, uint64_t serial)
{
	if (!serial) return nullptr;
	std::lock_guard<std::mutex> g(dev->lock);
	const int idx = (int)(serial % E264Device::NEV);
	return dev->sub_serial[idx] == serial ? dev->sub_ev[idx] : nullptr;
}
// An event handle read under dev->lock is queried or waited for OUTSIDE it, and ring entry serial % NEV is the next one next_serial() records
// again -- possibly for ANOTHER lane: a "done" answer only counts if the entry still belongs to the serial and lane it was read for once the call
// has returned (asked here, under the lock again); otherwise the answer is about somebody else's marker and nothing may be cached from it.
static bool serial_current(E264Device *dev, uint64_t serial, int lane)
{
	std::lock_guard<std::mutex> g(dev->lock);
	const int idx = (int)(serial % E264Device::NEV);
	return dev->sub_serial[idx] == serial && dev->sub_lane[idx] == lane;
}
// Has submission `serial` of lane `lane` left the GPU?  (serial 0: nothing was ever submitted)
static bool serial_retired(E264Device *dev, uint64_t serial, int lane)
{
	if (!serial) return true;
	std::atomic<uint64_t> &seen = dev->lane_retired[lane];
	if (serial <= seen.load(std::memory_order_relaxed)) return true; // no lock, no driver call: somebody saw this lane get past it
	hipEvent_t ev = serial_event(dev, serial);
	if (ev) {
		if (hipEventQuery(ev) != hipSuccess) { (void)hipGetLastError(); return false; }
		if (serial_current(dev, serial, lane)) { raise_serial(seen, serial); return true; }
		// re-recorded while we asked: the ring has wrapped past this serial, fall through to the wrapped path
	}
	// the event ring has wrapped past this serial.  A lane runs its work in order: a NEWER entry of the same lane that has retired proves
	// this one has (a continuously busy lane is never idle, hipStreamQuery alone would keep old blocks parked for good).  ONE query: the
	// oldest such entry still in the ring, picked under the lock, asked outside it (round 4 asked up to 64 under the lock, per parked block).
	hipEvent_t probe = nullptr;
	uint64_t probe_serial = 0;
	{
		std::lock_guard<std::mutex> g(dev->lock);
		for (int i = 0; i < E264Device::NEV; i++)
			if (dev->sub_serial[i] > serial && dev->sub_lane[i] == lane && dev->sub_ev[i] && (!probe || dev->sub_serial[i] < probe_serial)) { probe = dev->sub_ev[i]; probe_serial = dev->sub_serial[i]; }
	}
	if (probe && hipEventQuery(probe) == hipSuccess && serial_current(dev, probe_serial, lane)) { raise_serial(seen, probe_serial); return true; }
	(void)hipGetLastError(); // (hipErrorNotReady is not an error to keep)
	return hipStreamQuery(dev->q[lane]) == hipSuccess;
}
// Blocks until it has: the submission's own event, else (ring wrapped) the lane -- never the device.
static int serial_wait(E264Device *dev, uint64_t serial, int lane)
{
	if (!serial) return 0;
	hipEvent_t ev = serial_event(dev, serial);
	if (ev) {
		HIPCHK(hipEventSynchronize(ev), EIO);
		if (serial_current(dev, serial, lane)) return 0; // (else the entry was recorded again, for another lane, while we waited)
	}
	HIPCHK(hipStreamSynchronize(dev->q[lane]), EIO);
	return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// memory recycler
// ---------------------------------------------------------------------------------------------------------------------
static void *mem_raw(size_t bytes, bool host)
{
	void *p = nullptr;
	if ((host ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes)) == hipSuccess) return p;
	(void)hipGetLastError();
	return nullptr;
}
static void mem_free(const std::vector<E264Device::Parked> &blocks) // back to the driver for real (this drains the device's queues)
{
	for (auto &k : blocks) { if (k.host) hipHostFree(k.p); else hipFree(k.p); }
}
// (park_lock held) takes up to `max` parked blocks whose submission has retired off the list
static std::vector<E264Device::Parked> take_retired(E264Device *dev, size_t max)
{
	std::vector<E264Device::Parked> drop;
	for (size_t i = 0; i < dev->parked.size() && drop.size() < max;) {
		if (serial_retired(dev, dev->parked[i].serial, dev->parked[i].lane)) { drop.push_back(dev->parked[i]); dev->parked.erase(dev->parked.begin() + (ptrdiff_t)i); }
		else i++;
	}
	return drop;
}
static void *mem_acquire(E264Device *dev, size_t bytes, bool host)
{
	{
		std::lock_guard<std::mutex> g(dev->park_lock);
		for (size_t i = 0; i < dev->parked.size(); i++) {
			E264Device::Parked &k = dev->parked[i];
			if (k.host == host && k.bytes == bytes && serial_retired(dev, k.serial, k.lane)) {
				void *p = k.p;
				dev->parked.erase(dev->parked.begin() + (ptrdiff_t)i);
				return p;
			}
		}
	}
	if (void *p = mem_raw(bytes, host)) return p;
	// out of memory with blocks of other sizes parked (SPS size changes, many open / close cycles): the retired ones go back to the
	// driver (the price of running out), then once more
	dev->park_lock.lock();
	const std::vector<E264Device::Parked> drop = take_retired(dev, SIZE_MAX);
	dev->park_lock.unlock();
	if (drop.empty()) return nullptr;
	mem_free(drop);
	return mem_raw(bytes, host);
}
// `serial` / `lane`: the last submission that may touch the block (0: none)
static void mem_release(E264Device *dev, void *p, size_t bytes, bool host, uint64_t serial, int lane)
{
	if (!p) return;
	std::vector<E264Device::Parked> drop;
	{
		std::lock_guard<std::mutex> g(dev->park_lock);
		dev->parked.push_back({p, bytes, serial, lane, host});
		if (dev->parked.size() > E264Device::PARK_MAX) drop = take_retired(dev, E264Device::PARK_MAX / 4); // the oldest retired blocks really go (rare)
	}
	mem_free(drop);
}

// Gives the blocks of a GrowBuf back: parked behind `serial` of `lane`, the last submission that may touch them (0: nothing in flight does).
static void buf_release(E264Device *dev, GrowBuf &b, uint64_t serial = 0, int lane = 0)
{
	mem_release(dev, b.h, b.h_bytes, true, serial, lane);
	mem_release(dev, b.d, b.d_bytes, false, serial, lane);
	b = GrowBuf();
}
// Releases the old blocks as above and takes new ones of h_bytes / d_bytes (0: no such block) for `cap` units.  A failure leaves the buffer empty.
static int buf_grow(E264Device *dev, GrowBuf &b, size_t cap, size_t h_bytes, size_t d_bytes, const char *what_h, const char *what_d, uint64_t serial = 0, int lane = 0)
{
	buf_release(dev, b, serial, lane);
	if (h_bytes && !(b.h = (uint8_t *)mem_acquire(dev, h_bytes, true))) return fail(ENOMEM, what_h);
	if (d_bytes && !(b.d = (uint8_t *)mem_acquire(dev, d_bytes, false))) { mem_release(dev, b.h, h_bytes, true, 0, 0); b.h = nullptr; return fail(ENOMEM, what_d); }
	b.cap = cap; b.h_bytes = h_bytes; b.d_bytes = d_bytes;
	return 0;
}

API int e264hip_device_open(int ordinal, E264Device **out)
{
	if (!out) return fail(EINVAL, "null out");
	if (ablation_build_refused()) {
		snprintf(e264_err, sizeof(e264_err), "this library is a timing-ablation build (%s): its samples are wrong by design; set E264_ALLOW_ABLATION=1 to use it", e264_kernel_build_flags());
		return ENOTSUP;
	}
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(ENODEV, "no HIP device");
	if (ordinal < 0 || ordinal >= n) return fail(ENODEV, "device ordinal out of range");
	hipDeviceProp_t prop;
	HIPCHK(hipGetDeviceProperties(&prop, ordinal), EIO);
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
		snprintf(e264_err, sizeof(e264_err), "device %d is %s, this back end is built for gfx950 only", ordinal, prop.gcnArchName);
		return ENODEV;
	}
	E264Device *d = new (std::nothrow) E264Device();
	if (!d) return fail(ENOMEM, "device object");
	d->ordinal = ordinal;
	d->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	d->waves = 108; // round 4: e264_deblock2_kernel, 8 waves that take luma groups (8 rows) and chroma groups (15 rows) from one list: 0.99 - 1.02 ms against
	// 1.02 - 1.03 for the mixed waves below (profiles/r04_ablations.txt item 7).  Before (waves = 8, e264_deblock_kernel): 40 macroblock rows in flight (all the LDS takes: 154 KB); since the samples are fetched four macroblocks at a time 8 waves beat
	              // 7 (1.081 -> 1.051 ms per 256 x 1080p; round 2, one macroblock per fetch: 7 was the optimum)
	d->intra_waves = 16; // 16 rows in flight: 1.6 -> 1.1 ms per 256-frame launch (the intra kernel fits 128 VGPRs)
	d->ktiming = false; d->kev_used = 0;
	d->upload_queue = 1;
	for (int i = 0; i < E264Device::NQ; i++) { d->q[i] = nullptr; d->lane_ev[i] = nullptr; }
	if (hipSetDevice(ordinal) != hipSuccess) { delete d; return fail(EIO, "hipSetDevice"); }
	for (int i = 0; i < E264Device::NQ; i++)
		if (hipStreamCreateWithFlags(&d->q[i], hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&d->lane_ev[i], hipEventDisableTiming) != hipSuccess) {
			for (int k = 0; k <= i; k++) { if (d->q[k]) hipStreamDestroy(d->q[k]); if (d->lane_ev[k]) hipEventDestroy(d->lane_ev[k]); }
			delete d;
			return fail(EIO, "hipStreamCreate");
		}
	for (int i = 0; i < 16; i++)
		hipEventCreate(&d->ev[i]);
	d->split_intra = 1; d->split_planes = 1;
	d->side_queue = 0; // measured: no gain (profiles/r01k_ablation_breakdown.txt), off by default
	for (int i = 0; i < E264Device::NQ; i++) { d->q2[i] = nullptr; d->forked[i] = d->joined[i] = nullptr; }
	// The runtime deals its hardware queues (four by default, GPU_MAX_HW_QUEUES) to HIP streams in the order they are made: lane 0's second queue, the download
	// queue and the upload queue come right after the lanes, as in every round so far; the other lanes' second queues LAST (made in front of qc / qup they pushed the
	// download queue onto lane 0's hardware queue: one stream through edge264.h 1.03 -> 1.62 ms per picture, gpurun_out/r06f)
	auto make_q2 = [&](int i) {
		return hipStreamCreateWithFlags(&d->q2[i], hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&d->forked[i], hipEventDisableTiming) == hipSuccess &&
			hipEventCreateWithFlags(&d->joined[i], hipEventDisableTiming) == hipSuccess;
	};
	bool q2_ok = make_q2(0);
	if (hipStreamCreateWithFlags(&d->qc, hipStreamNonBlocking) != hipSuccess) d->qc = nullptr; // downloads then share the lane
	if (hipStreamCreateWithFlags(&d->qup, hipStreamNonBlocking) != hipSuccess) d->qup = nullptr; // uploads then share the lane
	for (int i = 1; i < E264Device::NQ && q2_ok; i++) q2_ok = make_q2(i);
	if (!q2_ok) // not fatal: the options that need a second queue then stay off
		for (int i = 0; i < E264Device::NQ; i++) {
			if (d->q2[i]) hipStreamDestroy(d->q2[i]);
			if (d->forked[i]) hipEventDestroy(d->forked[i]);
			if (d->joined[i]) hipEventDestroy(d->joined[i]);
			d->q2[i] = nullptr; d->forked[i] = d->joined[i] = nullptr;
		}
	for (int i = 0; i < E264Device::NEV; i++)
		if (hipEventCreateWithFlags(&d->sub_ev[i], E264_WAIT_EVENT) != hipSuccess) d->sub_ev[i] = nullptr;
	*out = d;
	return 0;
}

API int e264hip_device_sync(E264Device *dev)
{
	if (!dev) return fail(EINVAL, "null device");
	if (set_device(dev)) return EIO;
	if (dev->qup) HIPCHK(hipStreamSynchronize(dev->qup), EIO);
	for (int i = 0; i < E264Device::NQ; i++)
		HIPCHK(hipStreamSynchronize(dev->q[i]), EIO);
	for (int i = 0; i < E264Device::NQ; i++)
		if (dev->q2[i]) HIPCHK(hipStreamSynchronize(dev->q2[i]), EIO);
	return 0;
}

API void e264hip_device_close(E264Device *dev)
{
	if (!dev) return;
	hipSetDevice(dev->ordinal);
	e264hip_device_sync(dev);
	for (int i = 0; i < 16; i++) hipEventDestroy(dev->ev[i]);
	for (auto &p : dev->kev) { for (int i = 0; i < 5; i++) hipEventDestroy(p.e[i]); for (int i = 0; i < 2; i++) hipEventDestroy(p.a[i]); }
	for (int i = 0; i < E264Device::NQ; i++) {
		if (dev->q2[i]) hipStreamDestroy(dev->q2[i]);
		if (dev->forked[i]) hipEventDestroy(dev->forked[i]);
		if (dev->joined[i]) hipEventDestroy(dev->joined[i]);
	}
	for (auto &jr : dev->jring) {
		buf_release(dev, jr.jobs); buf_release(dev, jr.pkt); buf_release(dev, jr.xp); // (parked: freed below)
		if (jr.done) hipEventDestroy(jr.done);
		if (jr.up) hipEventDestroy(jr.up);
	}
	mem_free(dev->parked);
	dev->parked.clear();
	if (dev->qc) { hipStreamSynchronize(dev->qc); hipStreamDestroy(dev->qc); }
	if (dev->qup) hipStreamDestroy(dev->qup);
	for (int i = 0; i < E264Device::NEV; i++) if (dev->sub_ev[i]) hipEventDestroy(dev->sub_ev[i]);
	for (int i = 0; i < E264Device::NQ; i++) { hipStreamDestroy(dev->q[i]); hipEventDestroy(dev->lane_ev[i]); }
	delete dev;
}

API int e264hip_set_option(E264Device *dev, const char *name, int value)
{
	if (!dev || !name) return -1;
	if (!strcmp(name, "split_planes")) {
		int prev = dev->split_planes;
		dev->split_planes = value != 0;
		return prev;
	}
	if (!strcmp(name, "split_intra")) {
		int prev = dev->split_intra;
		dev->split_intra = value == 2 ? 2 : value != 0; // 2: also with more than two lanes in use (for runs with GPU_MAX_HW_QUEUES raised)
		return prev;
	}
	if (!strcmp(name, "side_queue")) {
		int prev = dev->side_queue;
		dev->side_queue = dev->q2[0] ? (value == 1 || value == 2 ? value : 0) : 0; // 1: beside the prediction kernel, 2: beside the intra kernel
		return prev;
	}
	if (!strcmp(name, "upload_queue")) {
		int prev = dev->upload_queue;
		dev->upload_queue = value != 0;
		return prev;
	}
	const bool intra = !strcmp(name, "intra_waves");
	if (intra || !strcmp(name, "waves")) {
		int &option = intra ? dev->intra_waves : dev->waves;
		const int prev = option;
		const E264Form *f = e264_form(intra, value);
		if (f && !f->exists) return -1; // a kernel this build does not have (waves 110, 112 without E264_DBK_GS = 2): refused, setting kept, instead of silently running as 108
		if (f) option = value; // anything else keeps the setting
		return prev;
	}
	return -1;
}

API int e264hip_stream_open(E264Device *dev, E264Stream **out)
{
	if (!dev || !out) return fail(EINVAL, "null argument");
	if (set_device(dev)) return EIO;
	E264Stream *s = new (std::nothrow) E264Stream();
	if (!s) return fail(ENOMEM, "stream object");
	memset(s, 0, sizeof(*s));
	s->dev = dev;
	s->d_table = (uint8_t **)mem_acquire(dev, sizeof(uint8_t *) * E264_MAX_SLOTS, false);
	s->tab_pin = (uint8_t **)mem_acquire(dev, sizeof(uint8_t *) * E264_MAX_SLOTS * E264Stream::NTAB, true);
	if (!s->d_table || !s->tab_pin) {
		mem_release(dev, s->d_table, sizeof(uint8_t *) * E264_MAX_SLOTS, false, 0, 0);
		mem_release(dev, s->tab_pin, sizeof(uint8_t *) * E264_MAX_SLOTS * E264Stream::NTAB, true, 0, 0);
		delete s;
		return fail(ENOMEM, "slot table");
	}
	hipMemsetAsync(s->d_table, 0, sizeof(uint8_t *) * E264_MAX_SLOTS, lane_of(s));
	dev->lane_streams[0].fetch_add(1, std::memory_order_relaxed);
	*out = s;
	return 0;
}

API int e264hip_stream_bind_lane(E264Stream *s, int lane)
{
	if (!s || lane < 0 || lane >= E264Device::NQ) return fail(EINVAL, "stream_bind_lane");
	if (lane == s->lane) return 0;
	if (set_device(s->dev)) return EIO;
	// what the old lane still has queued for this stream (table updates, fills, submissions) must be over before the new one starts
	HIPCHK(hipStreamSynchronize(lane_of(s)), EIO);
	s->dev->lane_streams[lane].fetch_add(1, std::memory_order_relaxed);
	s->dev->lane_streams[s->lane].fetch_sub(1, std::memory_order_relaxed);
	s->lane = lane;
	return 0;
}

// Waits for what THIS stream has submitted (edge264_flush, src/edge264.c:261-270), not for the device.
API int e264hip_stream_flush(E264Stream *s)
{
	if (!s) return fail(EINVAL, "null stream");
	if (set_device(s->dev)) return EIO;
	if (!s->last_serial) { HIPCHK(hipStreamSynchronize(lane_of(s)), EIO); return 0; } // fills / uploads only
	return serial_wait(s->dev, s->last_serial, s->lane);
}

API void e264hip_stream_close(E264Stream *s)
{
	if (!s) return;
	E264Device *dev = s->dev;
	set_device(dev);
	// everything THIS stream has queued on its lane (submissions, fills, table updates) -- not the device, not the other lanes
	hipEvent_t end = nullptr;
	if (hipEventCreateWithFlags(&end, E264_WAIT_EVENT) == hipSuccess && hipEventRecord(end, lane_of(s)) == hipSuccess) hipEventSynchronize(end);
	else hipStreamSynchronize(lane_of(s));
	if (end) hipEventDestroy(end);
	for (int i = 0; i < E264_MAX_SLOTS; i++) {
		mem_release(dev, s->h_table[i], s->slot_bytes[i] + 64, false, 0, 0);
		mem_release(dev, s->mirror[i], s->slot_bytes[i], true, 0, 0);
	}
	for (auto &st : s->stage) {
		buf_release(dev, st);
		mem_release(dev, st.d_job, sizeof(E264Job), false, 0, 0);
		if (st.done) hipEventDestroy(st.done);
	}
	buf_release(dev, s->dbk);
	buf_release(dev, s->expand);
	if (s->dl_done) hipEventDestroy(s->dl_done);
	for (int i = 0; i < E264Stream::NTAB; i++)
		if (s->tab_ev[i]) hipEventDestroy(s->tab_ev[i]);
	mem_release(dev, s->tab_pin, sizeof(uint8_t *) * E264_MAX_SLOTS * E264Stream::NTAB, true, 0, 0);
	mem_release(dev, s->d_table, sizeof(uint8_t *) * E264_MAX_SLOTS, false, 0, 0);
	dev->lane_streams[s->lane].fetch_sub(1, std::memory_order_relaxed);
	delete s;
}

// The slot table follows the stream's lane: enqueued after every kernel that still reads the old one, before any that
// needs the new one.  Asynchronous (pinned ring); the host waits only if it laps its own ring.
static int push_table(E264Stream *s)
{
	const int k = s->tab_next;
	s->tab_next = (k + 1) % E264Stream::NTAB;
	if (!s->tab_ev[k] && hipEventCreateWithFlags(&s->tab_ev[k], E264_WAIT_EVENT) != hipSuccess) { s->tab_ev[k] = nullptr; return fail(EIO, "hipEventCreate"); }
	if (s->tab_busy[k]) { HIPCHK(hipEventSynchronize(s->tab_ev[k]), EIO); s->tab_busy[k] = false; }
	uint8_t **pin = s->tab_pin + (size_t)k * E264_MAX_SLOTS;
	memcpy(pin, s->h_table, sizeof(uint8_t *) * E264_MAX_SLOTS);
	HIPCHK(hipMemcpyAsync(s->d_table, pin, sizeof(uint8_t *) * E264_MAX_SLOTS, hipMemcpyHostToDevice, lane_of(s)), EIO);
	HIPCHK(hipEventRecord(s->tab_ev[k], lane_of(s)), EIO);
	s->tab_busy[k] = true;
	return 0;
}

API int e264hip_frame_alloc(E264Stream *s, int slot, size_t samples_bytes, void **host_mirror)
{
	if (!s || slot < 0 || slot >= E264_MAX_SLOTS || samples_bytes == 0) return fail(EINVAL, "frame_alloc arguments");
	if (set_device(s->dev)) return EIO;
	if (s->h_table[slot]) e264hip_frame_free(s, slot);
	// +64: the MC fast path reads whole dwords up to 3 bytes past a 9-sample span (like the
	// reference's +16 over-read margin, src/edge264_headers.c:115)
	s->h_table[slot] = (uint8_t *)mem_acquire(s->dev, samples_bytes + 64, false);
	if (!s->h_table[slot]) return fail(ENOMEM, "hipMalloc frame");
	s->slot_bytes[slot] = samples_bytes;
	s->slot_serial[slot] = 0;
	if (host_mirror) {
		s->mirror[slot] = mem_acquire(s->dev, samples_bytes, true);
		if (!s->mirror[slot]) {
			mem_release(s->dev, s->h_table[slot], samples_bytes + 64, false, 0, 0); s->h_table[slot] = nullptr;
			return fail(ENOMEM, "hipHostMalloc mirror");
		}
		*host_mirror = s->mirror[slot];
	}
	return push_table(s);
}

API void e264hip_frame_free(E264Stream *s, int slot)
{
	if (!s || slot < 0 || slot >= E264_MAX_SLOTS || !s->h_table[slot]) return;
	set_device(s->dev);
	// A host batch naming this stream may be under assembly on another thread (e264_multi's submitter: it has read the stream's slot pointers for the
	// validation and not launched yet): the free waits for that batch to be launched or refused ...
	std::lock_guard<std::mutex> bg(s->dev->batch_lock);
	// ... and kernels and fills already queued may still read or write the slot: it is parked until the stream's latest work has retired
	// behind the lane's CURRENT tail (a marker of its own), not s->last_serial: a batch the submitter thread has just launched may not have
	// published its serial to the stream yet (the block could be recycled while that batch still used it)
	mem_release(s->dev, s->h_table[slot], s->slot_bytes[slot] + 64, false, mark_lane(s->dev, s->lane), s->lane);
	mem_release(s->dev, s->mirror[slot], s->slot_bytes[slot], true, 0, 0); // downloads are synchronous: nothing in flight
	s->h_table[slot] = nullptr; s->mirror[slot] = nullptr; s->slot_bytes[slot] = 0; s->slot_serial[slot] = 0;
	push_table(s);
}

API void *e264hip_frame_device_ptr(E264Stream *s, int slot)
{
	if (!s || slot < 0 || slot >= E264_MAX_SLOTS) return nullptr;
	return s->h_table[slot];
}

API int e264hip_frame_fill(E264Stream *s, int slot, int value)
{
	if (!s || slot < 0 || slot >= E264_MAX_SLOTS || !s->h_table[slot]) return fail(EINVAL, "frame_fill slot");
	if (set_device(s->dev)) return EIO;
	HIPCHK(hipMemsetAsync(s->h_table[slot], value, s->slot_bytes[slot], lane_of(s)), EIO);
	const uint64_t serial = mark_lane(s->dev, s->lane); // the fill has a serial and an event of its own
	publish_serial(s, slot, serial);
	return 0;
}

API int e264hip_frame_upload(E264Stream *s, int slot, const void *src, size_t bytes)
{
	if (!s || slot < 0 || slot >= E264_MAX_SLOTS || !s->h_table[slot] || bytes > s->slot_bytes[slot]) return fail(EINVAL, "frame_upload");
	if (set_device(s->dev)) return EIO;
	HIPCHK(hipMemcpyAsync(s->h_table[slot], src, bytes, hipMemcpyHostToDevice, lane_of(s)), EIO);
	HIPCHK(hipStreamSynchronize(lane_of(s)), EIO);
	s->slot_serial[slot] = 0;
	return 0;
}

// the stream's scratch for pictures of n_mbs macroblocks and, for a wire packet (area != 0), its expansion buffer
static int ensure_scratch(E264Stream *s, int n_mbs, size_t area = 0)
{
	// (queued kernels may still use the old blocks: parked behind the lane's tail, as frame_free)
	if (s->dbk.cap < (size_t)n_mbs && buf_grow(s->dev, s->dbk, (size_t)n_mbs, 0, E264_SCRATCH_BYTES(n_mbs), nullptr, "hipMalloc deblock parameters", mark_lane(s->dev, s->lane), s->lane)) return ENOMEM;
	if (s->expand.cap >= area) return 0;
	const size_t cap = (area + area / 4 + 65535) & ~(size_t)65535; // the motion section varies from picture to picture
	return buf_grow(s->dev, s->expand, cap, 0, cap, nullptr, "hipMalloc expansion buffer", mark_lane(s->dev, s->lane), s->lane);
}

// The highest lane that has a live stream (0 if none): what the rules below mean by "the lanes in use"
static int highest_lane_in_use(E264Device *dev)
{
	for (int i = E264Device::NQ - 1; i > 0; i--)
		if (dev->lane_streams[i].load(std::memory_order_relaxed) > 0) return i;
	return 0;
}

// Launches the kernels over a job table that already lives in HBM, on compute lane `lane`.
// in: the submission's part of the planner's input (n .. expand); the device's part is filled here
static int launch(E264Device *dev, int lane, const E264Job *d_jobs, int max_mbs, int max_tiles, E264PlanIn in, uint64_t *serial_out = nullptr)
{
	std::lock_guard<std::mutex> g(dev->lock);
	static const int alone_env = getenv("E264_PLANES_ALONE") ? atoi(getenv("E264_PLANES_ALONE")) : 0; // (for A/B)
	in.split_planes = dev->split_planes; in.split_intra = dev->split_intra; in.side_queue = dev->side_queue; in.waves = dev->waves; in.intra_waves = dev->intra_waves;
	in.n_cus = dev->n_cus; in.max_lane = highest_lane_in_use(dev); in.has_q2 = dev->q2[lane] != nullptr; in.planes_alone = alone_env;
	E264Plan plan;
	e264_plan(in, plan);
	hipEvent_t *marks = nullptr;
	E264Fork fork = {dev->q2[lane], dev->forked[lane], dev->joined[lane], nullptr};
	if (dev->ktiming) {
		if (dev->kev_used == dev->kev.size()) {
			E264Device::Marks m;
			for (int i = 0; i < 5; i++) hipEventCreate(&m.e[i]);
			for (int i = 0; i < 2; i++) hipEventCreate(&m.a[i]);
			dev->kev.push_back(m);
		}
		E264Device::Marks &m = dev->kev[dev->kev_used++];
		m.side = plan.param_where != E264_PARAM_ON_LANE; // (the parameter kernel's own marks; in a split submission it stays on the lane and the intra phase [2..3] holds the join)
		marks = m.e; fork.amarks = m.a;
	}
	HIPCHK(e264_launch_frames(d_jobs, in.n, max_mbs, max_tiles, plan, dev->q[lane], marks, fork), EIO);
	e264_plan_counts(plan, dev->launch_counts);
	const uint64_t serial = next_serial(dev, lane);
	if (serial_out) *serial_out = serial;
	return 0;
}

// Blocks until the submission that wrote `slot` last has retired (not until the device is idle).
static int wait_slot(E264Stream *s, int slot)
{
	if (!s->slot_serial[slot]) { // filled / uploaded outside a submission: the stream's lane
		HIPCHK(hipStreamSynchronize(lane_of(s)), EIO);
		return 0;
	}
	return serial_wait(s->dev, s->slot_serial[slot], s->lane);
}

// The next slot of the stream's staging ring, large enough for max_bytes: pinned host + device buffer + job slot + event.
static E264Stream::Stage *stage_prepare(E264Stream *s, size_t max_bytes)
{
	E264Stream::Stage &st = s->stage[s->stage_next];
	if (st.busy) { hipEventSynchronize(st.done); st.busy = false; }
	if (!st.done && hipEventCreateWithFlags(&st.done, E264_WAIT_EVENT) != hipSuccess) { st.done = nullptr; fail(EIO, "hipEventCreate"); return nullptr; }
	if (!st.d_job && !(st.d_job = (E264Job *)mem_acquire(s->dev, sizeof(E264Job), false))) { fail(ENOMEM, "job slot"); return nullptr; }
	const size_t cap = (max_bytes + 65535) & ~(size_t)65535;
	if (st.cap < max_bytes && buf_grow(s->dev, st, cap, cap + 64, cap, "pinned packet buffer", "device packet buffer")) return nullptr; // (not busy: nothing in flight reads the old blocks)
	return &st;
}

API void *e264hip_packet_buffer(E264Stream *s, size_t max_bytes)
{
	if (!s || set_device(s->dev)) return nullptr;
	E264Stream::Stage *st = stage_prepare(s, max_bytes);
	return st ? st->h : nullptr;
}

// entry i of a batch's streams: on this device, on the lane of the first ...
static int check_lane(E264Device *dev, E264Stream *const *streams, int i)
{
	if (!streams[i] || streams[i]->dev != dev) return fail(EINVAL, "batch entry");
	if (streams[i]->lane != streams[0]->lane) return fail(EINVAL, "the streams of a batch must be bound to one compute lane");
	return 0;
}
// ... and not there before: two jobs of one stream would share its DPB and parameter buffer inside one launch
static int check_once(E264Stream *const *streams, int i)
{
	for (int j = 0; j < i; j++)
		if (streams[j] == streams[i]) return fail(EINVAL, "a stream may contribute one frame per batch");
	return 0;
}
// The job table's order is the launcher's to choose: pictures without prediction work (I pictures) LAST, so that a mixed batch can start their intra pass
// beside the others' parameter and prediction kernels (E264PlanIn.n_nopred = back)
struct JobOrder { int n, front = 0, back = 0; int slot(bool pred_work) { return pred_work ? front++ : n - 1 - back++; } };
// the submission's part of the planner's input: n pictures, the last n_nopred of the table without prediction work, the caller's mode (E264_RUN_ALL bits) and
// what the validation of every packet says (some holds an inter or PCM macroblock / predicts from list 1)
static E264PlanIn submission(int n, int n_nopred, int mode, bool pred_work, bool has_l1)
{
	E264PlanIn in = {};
	in.n = n; in.n_nopred = n_nopred;
	in.recon = (mode & E264_RUN_RECON) != 0; in.deblock = (mode & E264_RUN_DEBLOCK) != 0;
	in.pred_work = pred_work; in.has_l1 = has_l1;
	return in;
}

API int e264hip_frame_submit(E264Stream *s, const void *packet, size_t bytes)
{
	if (!s) return fail(EINVAL, "null stream");
	E264PacketInfo pi;
	int r = e264_check_header(packet, bytes, &pi);
	if (r) return r;
	if (!s->h_table[pi.dst_slot]) return fail(EINVAL, "destination slot not allocated");
	if ((r = e264_check_records(packet, slots_of(s), &pi))) return r;
	if (set_device(s->dev)) return EIO;
	if ((r = ensure_scratch(s, pi.n_mbs(), pi.area))) return r;
	E264Stream::Stage *st = &s->stage[s->stage_next];
	if (packet == st->h && bytes > st->cap) return fail(EINVAL, "packet larger than the buffer e264hip_packet_buffer returned");
	if (packet != st->h) { // caller did not use our pinned buffer: stage it
		st = stage_prepare(s, bytes);
		if (!st) return ENOMEM;
		memcpy(st->h, packet, bytes);
	}
	s->stage_next = (s->stage_next + 1) & 3;
	hipStream_t q = lane_of(s);
	// the job record rides at the tail of the pinned staging buffer: tiny H2D on the same queue
	E264Job *job = (E264Job *)(st->h + st->cap); // pinned, lives as long as the staging slot
	job->packet = st->d; job->dpb = s->d_table; job->dbk = s->dbk.d; job->expand = pi.area ? s->expand.d : nullptr;
	hipError_t e = hipMemcpyAsync(st->d, st->h, bytes, hipMemcpyHostToDevice, q);
	if (e == hipSuccess) e = hipMemcpyAsync(st->d_job, job, sizeof(*job), hipMemcpyHostToDevice, q);
	uint64_t serial = 0;
	E264PlanIn in = submission(1, 0, E264_RUN_ALL, pi.pred_work, pi.has_l1);
	in.expand = pi.area != 0; // a wire packet: unfolded on the lane, in front of the four
	r = e == hipSuccess ? launch(s->dev, s->lane, st->d_job, pi.n_mbs(), e264_pred_tiles(pi.width_mbs, pi.height_mbs), in, &serial) : fail(EIO, "hipMemcpyAsync packet", e);
	// whatever was queued reads the staging slot: it is busy until the lane has passed this point, error or not
	hipEventRecord(st->done, q);
	st->busy = true;
	if (r) return r;
	publish_serial(s, pi.dst_slot, serial);
	return 0;
}

API int e264hip_frame_wait(E264Stream *s, int slot)
{
	if (!s || slot < 0 || slot >= E264_MAX_SLOTS) return fail(EINVAL, "frame_wait");
	if (!s->h_table[slot]) return fail(EINVAL, "frame_wait slot");
	if (set_device(s->dev)) return EIO;
	return wait_slot(s, slot);
}

API int e264hip_frame_download(E264Stream *s, int slot, void *dst, size_t bytes)
{
	if (!s || slot < 0 || slot >= E264_MAX_SLOTS || !s->h_table[slot]) return fail(EINVAL, "frame_download slot");
	if (set_device(s->dev)) return EIO;
	if (!dst) dst = s->mirror[slot];
	if (!dst) return fail(EINVAL, "no destination");
	if (bytes == 0 || bytes > s->slot_bytes[slot]) bytes = s->slot_bytes[slot];
	int r = wait_slot(s, slot); // the frame is final on the device; the copy runs beside whatever other decoders have queued since
	if (r) return r;
	hipStream_t qc = s->dev->qc ? s->dev->qc : lane_of(s);
	if (!s->dl_done && hipEventCreateWithFlags(&s->dl_done, E264_WAIT_EVENT) != hipSuccess) { s->dl_done = nullptr; return fail(EIO, "hipEventCreate"); }
	HIPCHK(hipMemcpyAsync(dst, s->h_table[slot], bytes, hipMemcpyDeviceToHost, qc), EIO);
	HIPCHK(hipEventRecord(s->dl_done, qc), EIO);
	HIPCHK(hipEventSynchronize(s->dl_done), EIO);
	return 0;
}

// Digests of n pictures (include/edge264_hip.h), one kernel on the streams' lane behind everything queued there.  The job table goes up and the results
// come down through ONE page-locked block [jobs | results] and one device block of the same shape, both from the recycler and back in it after the wait
// (sized for n rounded up to 64, so that calls of similar size find each other's blocks).  On the lane, under dev->lock: the table's copy, the clear of the
// results (the workgroups ADD to them), the kernel, the results' copy, and the call's own serial -- a lane mark as a fill takes, so that a slot freed while the
// kernel runs is parked behind it.  The wait is for that serial's event, outside the lock.
// The slots' pointers and sizes are read before that lock is taken and without batch_lock: the caller drives these streams, as for a submission (a frame_free of
// another thread between the checks and the launch would still leave the block alive -- parked behind a later mark -- but the picture in it is no longer the caller's).
API int e264hip_digest_batch(E264Device *dev, E264Stream *const *streams, const int *slots, const E264View *views, int n, uint64_t *out)
{
	if (!dev || n < 0 || n > E264_DIGEST_MAX_BATCH) return fail(EINVAL, "digest_batch: null device or n outside 0..4096");
	if (n == 0) return 0;
	if (!streams || !slots || !views || !out) return fail(EINVAL, "digest_batch: null argument");
	int r;
	for (int i = 0; i < n; i++) {
		if ((r = check_lane(dev, streams, i))) return r;
		if (slots[i] < 0 || slots[i] >= E264_MAX_SLOTS || !streams[i]->h_table[slots[i]]) return fail(EINVAL, "digest_batch: slot out of range or not allocated");
		if ((r = e264hip_view_check(&views[i], streams[i]->slot_bytes[slots[i]]))) return r;
	}
	if (set_device(dev)) return EIO;
	const int lane = streams[0]->lane;
	const size_t cap = ((size_t)n + 63) & ~(size_t)63, jobs_bytes = cap * sizeof(E264DigestJob), bytes = jobs_bytes + cap * 3 * sizeof(uint64_t);
	uint8_t *h = (uint8_t *)mem_acquire(dev, bytes, true), *d = h ? (uint8_t *)mem_acquire(dev, bytes, false) : nullptr;
	if (!d) { mem_release(dev, h, bytes, true, 0, 0); return fail(ENOMEM, "digest_batch: job table"); }
	E264DigestJob *jobs = (E264DigestJob *)h;
	uint32_t max_chunks = 1;
	for (int i = 0; i < n; i++) {
		jobs[i].base = streams[i]->h_table[slots[i]];
		jobs[i].slot_bytes = streams[i]->slot_bytes[slots[i]];
		jobs[i].view = views[i];
		jobs[i].chunks = e264_digest_chunks(&views[i]);
		max_chunks = std::max(max_chunks, jobs[i].chunks);
	}
	uint64_t serial;
	hipError_t e;
	{
		std::lock_guard<std::mutex> g(dev->lock);
		hipStream_t q = dev->q[lane];
		e = hipMemcpyAsync(d, h, (size_t)n * sizeof(E264DigestJob), hipMemcpyHostToDevice, q);
		if (e == hipSuccess) e = hipMemsetAsync(d + jobs_bytes, 0, (size_t)n * 3 * sizeof(uint64_t), q);
		if (e == hipSuccess) e = e264_launch_digest((const E264DigestJob *)d, n, max_chunks, (uint64_t *)(d + jobs_bytes), q);
		if (e == hipSuccess) e = hipMemcpyAsync(h + jobs_bytes, d + jobs_bytes, (size_t)n * 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, q);
		serial = next_serial(dev, lane); // (also after an error: whatever was queued reads the two blocks until the lane has passed this point)
	}
	r = e == hipSuccess ? serial_wait(dev, serial, lane) : fail(EIO, "digest_batch", e);
	if (!r) memcpy(out, h + jobs_bytes, (size_t)n * 3 * sizeof(uint64_t));
	mem_release(dev, h, bytes, true, serial, lane);
	mem_release(dev, d, bytes, false, serial, lane);
	return r;
}

API int e264hip_frame_digest(E264Stream *s, int slot, const E264View *view, uint64_t out[3])
{
	if (!s) return fail(EINVAL, "frame_digest: null stream");
	return e264hip_digest_batch(s->dev, &s, &slot, view, 1, out);
}

// Reduced previews of n pictures (include/edge264_hip.h), built like e264hip_digest_batch: one kernel on the streams' lane behind everything queued there; ONE
// page-locked block [jobs | previews] and one device block of the same shape, both from the recycler and back in it behind the call's own serial (jobs sized for
// n rounded up to 64, previews rounded up to 64 KiB, so that calls of similar size find each other's blocks).  In the device block the pictures lie back to back,
// each rounded up to 16 bytes; the kernel writes every byte of every preview, so nothing is cleared in front.  On the lane, under dev->lock: the table's copy,
// the kernel, ONE copy of the previews down, the serial.  The wait is for that serial's event, outside the lock; then a memcpy per picture into `out`, whose
// bytes between the pictures are never touched.
API int e264hip_preview_batch(E264Device *dev, E264Stream *const *streams, const int *slots, const E264View *views, int n, int log2_factor, void *out, size_t pitch)
{
	if (!dev || n < 0 || n > E264_PREVIEW_MAX_BATCH) return fail(EINVAL, "preview_batch: null device or n outside 0..4096");
	if (n == 0) return 0;
	if (!streams || !slots || !views || !out) return fail(EINVAL, "preview_batch: null argument");
	if (log2_factor < 1 || log2_factor > 3) return fail(EINVAL, "preview_batch: log2_factor is none of 1, 2, 3");
	int r;
	size_t total = 0;
	for (int i = 0; i < n; i++) {
		if ((r = check_lane(dev, streams, i))) return r;
		if (slots[i] < 0 || slots[i] >= E264_MAX_SLOTS || !streams[i]->h_table[slots[i]]) return fail(EINVAL, "preview_batch: slot out of range or not allocated");
		if ((r = e264hip_view_check(&views[i], streams[i]->slot_bytes[slots[i]]))) return r;
		const size_t b = e264hip_preview_bytes(&views[i], log2_factor, nullptr); // (> 0: the view has samples; < 2^30)
		if (b > pitch) return fail(EINVAL, "preview_batch: pitch (or cap) smaller than a picture's preview");
		total += (b + 15) & ~(size_t)15;
		if (total > E264_PREVIEW_MAX_BYTES) return fail(EINVAL, "preview_batch: more than E264_PREVIEW_MAX_BYTES in one call");
	}
	if (set_device(dev)) return EIO;
	const int lane = streams[0]->lane;
	const size_t cap = ((size_t)n + 63) & ~(size_t)63, jobs_bytes = cap * sizeof(E264PreviewJob), bytes = jobs_bytes + ((total + 65535) & ~(size_t)65535);
	uint8_t *h = (uint8_t *)mem_acquire(dev, bytes, true), *d = h ? (uint8_t *)mem_acquire(dev, bytes, false) : nullptr;
	if (!d) { mem_release(dev, h, bytes, true, 0, 0); return fail(ENOMEM, "preview_batch: job table and previews"); }
	E264PreviewJob *jobs = (E264PreviewJob *)h;
	uint32_t max_chunks = 1;
	size_t at = jobs_bytes;
	for (int i = 0; i < n; i++) {
		jobs[i].base = streams[i]->h_table[slots[i]];
		jobs[i].slot_bytes = streams[i]->slot_bytes[slots[i]];
		jobs[i].view = views[i];
		jobs[i].dst = d + at;
		jobs[i].k = (uint32_t)log2_factor;
		jobs[i].chunks = e264_preview_chunks(&views[i], log2_factor);
		max_chunks = std::max(max_chunks, jobs[i].chunks);
		at += (e264hip_preview_bytes(&views[i], log2_factor, nullptr) + 15) & ~(size_t)15;
	}
	uint64_t serial;
	hipError_t e;
	{
		std::lock_guard<std::mutex> g(dev->lock);
		hipStream_t q = dev->q[lane];
		e = hipMemcpyAsync(d, h, (size_t)n * sizeof(E264PreviewJob), hipMemcpyHostToDevice, q);
		if (e == hipSuccess) e = e264_launch_preview((const E264PreviewJob *)d, n, max_chunks, q);
		if (e == hipSuccess) e = hipMemcpyAsync(h + jobs_bytes, d + jobs_bytes, total, hipMemcpyDeviceToHost, q);
		serial = next_serial(dev, lane); // (also after an error: whatever was queued reads the two blocks until the lane has passed this point)
	}
	r = e == hipSuccess ? serial_wait(dev, serial, lane) : fail(EIO, "preview_batch", e);
	if (!r)
		for (int i = 0; i < n; i++)
			memcpy((uint8_t *)out + (size_t)i * pitch, h + (jobs[i].dst - d), e264hip_preview_bytes(&views[i], log2_factor, nullptr));
	mem_release(dev, h, bytes, true, serial, lane);
	mem_release(dev, d, bytes, false, serial, lane);
	return r;
}

API int e264hip_frame_preview(E264Stream *s, int slot, const E264View *view, int log2_factor, void *out, size_t cap)
{
	if (!s) return fail(EINVAL, "frame_preview: null stream");
	return e264hip_preview_batch(s->dev, &s, &slot, view, 1, log2_factor, out, cap);
}

// Difference records of n pairs of pictures (include/edge264_hip.h), built like e264hip_digest_batch: one kernel on the streams' lane behind everything queued
// there; ONE page-locked block [jobs | records] and one device block of the same shape, both from the recycler and back in it behind the call's own serial (sized
// for n rounded up to 64).  On the lane, under dev->lock: the table's copy, ONE clear of the records (the workgroups add and max into them; `first` travels as
// ~first, so that zeros are its start too), the kernel, the records' copy, the serial.  The wait is for that serial's event, outside the lock; then the records go
// to `out` with every `first` turned round.
API int e264hip_diff_batch(E264Device *dev, E264Stream *const *streams_a, const int *slots_a, const E264View *views_a,
	E264Stream *const *streams_b, const int *slots_b, const E264View *views_b, int n, E264Diff *out)
{
	if (!dev || n < 0 || n > E264_DIFF_MAX_BATCH) return fail(EINVAL, "diff_batch: null device or n outside 0..4096");
	if (n == 0) return 0;
	if (!streams_a || !slots_a || !views_a || !streams_b || !slots_b || !views_b || !out) return fail(EINVAL, "diff_batch: null argument");
	int r;
	for (int i = 0; i < n; i++) {
		if ((r = check_lane(dev, streams_a, i)) || (r = check_lane(dev, streams_b, i))) return r;
		if (streams_b[i]->lane != streams_a[0]->lane) return fail(EINVAL, "the streams of a batch must be bound to one compute lane");
		if (slots_a[i] < 0 || slots_a[i] >= E264_MAX_SLOTS || !streams_a[i]->h_table[slots_a[i]] || slots_b[i] < 0 || slots_b[i] >= E264_MAX_SLOTS || !streams_b[i]->h_table[slots_b[i]])
			return fail(EINVAL, "diff_batch: slot out of range or not allocated");
		if ((r = e264hip_diff_check(&views_a[i], streams_a[i]->slot_bytes[slots_a[i]], &views_b[i], streams_b[i]->slot_bytes[slots_b[i]]))) return r;
	}
	if (set_device(dev)) return EIO;
	const int lane = streams_a[0]->lane;
	const size_t cap = ((size_t)n + 63) & ~(size_t)63, jobs_bytes = cap * sizeof(E264DiffJob), bytes = jobs_bytes + cap * sizeof(E264Diff);
	uint8_t *h = (uint8_t *)mem_acquire(dev, bytes, true), *d = h ? (uint8_t *)mem_acquire(dev, bytes, false) : nullptr;
	if (!d) { mem_release(dev, h, bytes, true, 0, 0); return fail(ENOMEM, "diff_batch: job table"); }
	E264DiffJob *jobs = (E264DiffJob *)h;
	uint32_t max_chunks = 1;
	for (int i = 0; i < n; i++) {
		jobs[i].base_a = streams_a[i]->h_table[slots_a[i]];
		jobs[i].slot_bytes_a = streams_a[i]->slot_bytes[slots_a[i]];
		jobs[i].base_b = streams_b[i]->h_table[slots_b[i]];
		jobs[i].slot_bytes_b = streams_b[i]->slot_bytes[slots_b[i]];
		jobs[i].view_a = views_a[i];
		jobs[i].view_b = views_b[i];
		jobs[i].chunks = e264_diff_chunks(&views_a[i]);
		max_chunks = std::max(max_chunks, jobs[i].chunks);
	}
	uint64_t serial;
	hipError_t e;
	{
		std::lock_guard<std::mutex> g(dev->lock);
		hipStream_t q = dev->q[lane];
		e = hipMemcpyAsync(d, h, (size_t)n * sizeof(E264DiffJob), hipMemcpyHostToDevice, q);
		if (e == hipSuccess) e = hipMemsetAsync(d + jobs_bytes, 0, (size_t)n * sizeof(E264Diff), q);
		if (e == hipSuccess) e = e264_launch_diff((const E264DiffJob *)d, n, max_chunks, (E264Diff *)(d + jobs_bytes), q);
		if (e == hipSuccess) e = hipMemcpyAsync(h + jobs_bytes, d + jobs_bytes, (size_t)n * sizeof(E264Diff), hipMemcpyDeviceToHost, q);
		serial = next_serial(dev, lane); // (also after an error: whatever was queued reads the two blocks until the lane has passed this point)
	}
	r = e == hipSuccess ? serial_wait(dev, serial, lane) : fail(EIO, "diff_batch", e);
	if (!r) {
		memcpy(out, h + jobs_bytes, (size_t)n * sizeof(E264Diff));
		for (int i = 0; i < n; i++)
			for (int p = 0; p < 3; p++)
				out[i].plane[p].first = ~out[i].plane[p].first; // (the kernel keeps ~first under a max)
	}
	mem_release(dev, h, bytes, true, serial, lane);
	mem_release(dev, d, bytes, false, serial, lane);
	return r;
}

API int e264hip_frame_diff(E264Stream *a, int slot_a, const E264View *view_a, E264Stream *b, int slot_b, const E264View *view_b, E264Diff *out)
{
	if (!a || !b) return fail(EINVAL, "frame_diff: null stream");
	return e264hip_diff_batch(a->dev, &a, &slot_a, view_a, &b, &slot_b, view_b, 1, out);
}

// Histogram records of n pictures (include/edge264_hip.h), built like e264hip_diff_batch: one kernel on the streams' lane behind everything queued there; ONE
// page-locked block [jobs | records] and one device block of the same shape, both from the recycler and back in it behind the call's own serial (sized for n
// rounded up to 64).  On the lane, under dev->lock: the table's copy, ONE clear of the records (the workgroups add into them), the kernel, the records' copy, the
// serial.  The wait is for that serial's event, outside the lock; then the records go to `out`.
API int e264hip_hist_batch(E264Device *dev, E264Stream *const *streams, const int *slots, const E264View *views, int n, E264Hist *out)
{
	if (!dev || n < 0 || n > E264_HIST_MAX_BATCH) return fail(EINVAL, "hist_batch: null device or n outside 0..4096");
	if (n == 0) return 0;
	if (!streams || !slots || !views || !out) return fail(EINVAL, "hist_batch: null argument");
	int r;
	for (int i = 0; i < n; i++) {
		if ((r = check_lane(dev, streams, i))) return r;
		if (slots[i] < 0 || slots[i] >= E264_MAX_SLOTS || !streams[i]->h_table[slots[i]]) return fail(EINVAL, "hist_batch: slot out of range or not allocated");
		if ((r = e264hip_view_check(&views[i], streams[i]->slot_bytes[slots[i]]))) return r;
	}
	if (set_device(dev)) return EIO;
	const int lane = streams[0]->lane;
	const size_t cap = ((size_t)n + 63) & ~(size_t)63, jobs_bytes = cap * sizeof(E264HistJob), bytes = jobs_bytes + cap * sizeof(E264Hist);
	uint8_t *h = (uint8_t *)mem_acquire(dev, bytes, true), *d = h ? (uint8_t *)mem_acquire(dev, bytes, false) : nullptr;
	if (!d) { mem_release(dev, h, bytes, true, 0, 0); return fail(ENOMEM, "hist_batch: job table"); }
	E264HistJob *jobs = (E264HistJob *)h;
	uint32_t max_chunks = 1;
	for (int i = 0; i < n; i++) {
		jobs[i].base = streams[i]->h_table[slots[i]];
		jobs[i].slot_bytes = streams[i]->slot_bytes[slots[i]];
		jobs[i].view = views[i];
		jobs[i].chunks = e264_hist_chunks(&views[i]);
		max_chunks = std::max(max_chunks, jobs[i].chunks);
	}
	uint64_t serial;
	hipError_t e;
	{
		std::lock_guard<std::mutex> g(dev->lock);
		hipStream_t q = dev->q[lane];
		e = hipMemcpyAsync(d, h, (size_t)n * sizeof(E264HistJob), hipMemcpyHostToDevice, q);
		if (e == hipSuccess) e = hipMemsetAsync(d + jobs_bytes, 0, (size_t)n * sizeof(E264Hist), q);
		if (e == hipSuccess) e = e264_launch_hist((const E264HistJob *)d, n, max_chunks, (E264Hist *)(d + jobs_bytes), q);
		if (e == hipSuccess) e = hipMemcpyAsync(h + jobs_bytes, d + jobs_bytes, (size_t)n * sizeof(E264Hist), hipMemcpyDeviceToHost, q);
		serial = next_serial(dev, lane); // (also after an error: whatever was queued reads the two blocks until the lane has passed this point)
	}
	r = e == hipSuccess ? serial_wait(dev, serial, lane) : fail(EIO, "hist_batch", e);
	if (!r) memcpy(out, h + jobs_bytes, (size_t)n * sizeof(E264Hist));
	mem_release(dev, h, bytes, true, serial, lane);
	mem_release(dev, d, bytes, false, serial, lane);
	return r;
}

API int e264hip_frame_hist(E264Stream *s, int slot, const E264View *view, E264Hist *out)
{
	if (!s) return fail(EINVAL, "frame_hist: null stream");
	return e264hip_hist_batch(s->dev, &s, &slot, view, 1, out);
}

// Block difference maps of n pairs of pictures (include/edge264_hip.h), the pairs checked like e264hip_diff_batch's and the maps carried like
// e264hip_preview_batch's previews: one kernel on the streams' lane behind everything queued there; ONE page-locked block [jobs | maps] and one device block of the
// same shape, both from the recycler and back in it behind the call's own serial (jobs sized for n rounded up to 64, maps rounded up to 64 KiB).  In the device
// block the maps lie back to back, each rounded up to 16 bytes; the kernel writes every record of every map, so nothing is cleared in front.  On the lane, under
// dev->lock: the table's copy, the kernel, ONE copy of the maps down, the serial.  The wait is for that serial's event, outside the lock; then a memcpy per pair
// into `out`, whose bytes between the maps are never touched.
API int e264hip_blockdiff_batch(E264Device *dev, E264Stream *const *streams_a, const int *slots_a, const E264View *views_a,
	E264Stream *const *streams_b, const int *slots_b, const E264View *views_b, int n, int log2_block, void *out, size_t pitch)
{
	if (!dev || n < 0 || n > E264_BLOCKDIFF_MAX_BATCH) return fail(EINVAL, "blockdiff_batch: null device or n outside 0..4096");
	if (n == 0) return 0;
	if (!streams_a || !slots_a || !views_a || !streams_b || !slots_b || !views_b || !out) return fail(EINVAL, "blockdiff_batch: null argument");
	int r;
	size_t total = 0;
	for (int i = 0; i < n; i++) {
		if ((r = check_lane(dev, streams_a, i)) || (r = check_lane(dev, streams_b, i))) return r;
		if (streams_b[i]->lane != streams_a[0]->lane) return fail(EINVAL, "the streams of a batch must be bound to one compute lane");
		if (slots_a[i] < 0 || slots_a[i] >= E264_MAX_SLOTS || !streams_a[i]->h_table[slots_a[i]] || slots_b[i] < 0 || slots_b[i] >= E264_MAX_SLOTS || !streams_b[i]->h_table[slots_b[i]])
			return fail(EINVAL, "blockdiff_batch: slot out of range or not allocated");
		if ((r = e264hip_blockdiff_check(&views_a[i], streams_a[i]->slot_bytes[slots_a[i]], &views_b[i], streams_b[i]->slot_bytes[slots_b[i]], log2_block))) return r;
		const size_t b = e264hip_blockdiff_bytes(&views_a[i], log2_block, nullptr); // (> 0: the view has samples and k is in range; < 2^31)
		if (b > pitch) return fail(EINVAL, "blockdiff_batch: pitch (or cap) smaller than a pair's map");
		total += (b + 15) & ~(size_t)15;
		if (total > E264_BLOCKDIFF_MAX_BYTES) return fail(EINVAL, "blockdiff_batch: more than E264_BLOCKDIFF_MAX_BYTES in one call");
	}
	if (set_device(dev)) return EIO;
	const int lane = streams_a[0]->lane;
	const size_t cap = ((size_t)n + 63) & ~(size_t)63, jobs_bytes = (cap * sizeof(E264BlockDiffJob) + 15) & ~(size_t)15, bytes = jobs_bytes + ((total + 65535) & ~(size_t)65535);
	uint8_t *h = (uint8_t *)mem_acquire(dev, bytes, true), *d = h ? (uint8_t *)mem_acquire(dev, bytes, false) : nullptr;
	if (!d) { mem_release(dev, h, bytes, true, 0, 0); return fail(ENOMEM, "blockdiff_batch: job table and maps"); }
	E264BlockDiffJob *jobs = (E264BlockDiffJob *)h;
	uint32_t max_chunks = 1;
	size_t at = jobs_bytes;
	for (int i = 0; i < n; i++) {
		jobs[i].base_a = streams_a[i]->h_table[slots_a[i]];
		jobs[i].slot_bytes_a = streams_a[i]->slot_bytes[slots_a[i]];
		jobs[i].base_b = streams_b[i]->h_table[slots_b[i]];
		jobs[i].slot_bytes_b = streams_b[i]->slot_bytes[slots_b[i]];
		jobs[i].view_a = views_a[i];
		jobs[i].view_b = views_b[i];
		jobs[i].dst = d + at;
		jobs[i].k = (uint32_t)log2_block;
		jobs[i].chunks = e264_blockdiff_chunks(&views_a[i], log2_block);
		max_chunks = std::max(max_chunks, jobs[i].chunks);
		at += (e264hip_blockdiff_bytes(&views_a[i], log2_block, nullptr) + 15) & ~(size_t)15;
	}
	uint64_t serial;
	hipError_t e;
	{
		std::lock_guard<std::mutex> g(dev->lock);
		hipStream_t q = dev->q[lane];
		e = hipMemcpyAsync(d, h, (size_t)n * sizeof(E264BlockDiffJob), hipMemcpyHostToDevice, q);
		if (e == hipSuccess) e = e264_launch_blockdiff((const E264BlockDiffJob *)d, n, max_chunks, q);
		if (e == hipSuccess) e = hipMemcpyAsync(h + jobs_bytes, d + jobs_bytes, total, hipMemcpyDeviceToHost, q);
		serial = next_serial(dev, lane); // (also after an error: whatever was queued reads the two blocks until the lane has passed this point)
	}
	r = e == hipSuccess ? serial_wait(dev, serial, lane) : fail(EIO, "blockdiff_batch", e);
	if (!r)
		for (int i = 0; i < n; i++)
			memcpy((uint8_t *)out + (size_t)i * pitch, h + (jobs[i].dst - d), e264hip_blockdiff_bytes(&views_a[i], log2_block, nullptr));
	mem_release(dev, h, bytes, true, serial, lane);
	mem_release(dev, d, bytes, false, serial, lane);
	return r;
}

API int e264hip_frame_blockdiff(E264Stream *a, int slot_a, const E264View *view_a, E264Stream *b, int slot_b, const E264View *view_b, int log2_block, void *out, size_t cap)
{
	if (!a || !b) return fail(EINVAL, "frame_blockdiff: null stream");
	return e264hip_blockdiff_batch(a->dev, &a, &slot_a, view_a, &b, &slot_b, view_b, 1, log2_block, out, cap);
}

// Block statistics maps of n pictures (include/edge264_hip.h), the pictures checked like e264hip_hist_batch's and the maps carried like
// e264hip_blockdiff_batch's: one kernel on the streams' lane behind everything queued there; ONE page-locked block [jobs | maps] and one device block of the
// same shape, both from the recycler and back in it behind the call's own serial (jobs sized for n rounded up to 64, maps rounded up to 64 KiB).  In the device
// block the maps lie back to back (a record is 16 bytes, so every map is 16-byte aligned); the kernel writes every record of every map, so nothing is cleared in
// front.  On the lane, under dev->lock: the table's copy, the kernel, ONE copy of the maps down, the serial.  The wait is for that serial's event, outside the
// lock; then a memcpy per picture into `out`, whose bytes between the maps are never touched.
API int e264hip_blockstat_batch(E264Device *dev, E264Stream *const *streams, const int *slots, const E264View *views, int n, int log2_block, void *out, size_t pitch)
{
	if (!dev || n < 0 || n > E264_BLOCKSTAT_MAX_BATCH) return fail(EINVAL, "blockstat_batch: null device or n outside 0..4096");
	if (n == 0) return 0;
	if (!streams || !slots || !views || !out) return fail(EINVAL, "blockstat_batch: null argument");
	int r;
	size_t total = 0;
	for (int i = 0; i < n; i++) {
		if ((r = check_lane(dev, streams, i))) return r;
		if (slots[i] < 0 || slots[i] >= E264_MAX_SLOTS || !streams[i]->h_table[slots[i]]) return fail(EINVAL, "blockstat_batch: slot out of range or not allocated");
		if ((r = e264hip_blockstat_check(&views[i], streams[i]->slot_bytes[slots[i]], log2_block))) return r;
		const size_t b = e264hip_blockstat_bytes(&views[i], log2_block, nullptr); // (> 0: the view has samples and k is in range; a multiple of 16)
		if (b > pitch) return fail(EINVAL, "blockstat_batch: pitch (or cap) smaller than a picture's map");
		total += b;
		if (total > E264_BLOCKSTAT_MAX_BYTES) return fail(EINVAL, "blockstat_batch: more than E264_BLOCKSTAT_MAX_BYTES in one call");
	}
	if (set_device(dev)) return EIO;
	const int lane = streams[0]->lane;
	const size_t cap = ((size_t)n + 63) & ~(size_t)63, jobs_bytes = (cap * sizeof(E264BlockStatJob) + 15) & ~(size_t)15, bytes = jobs_bytes + ((total + 65535) & ~(size_t)65535);
	uint8_t *h = (uint8_t *)mem_acquire(dev, bytes, true), *d = h ? (uint8_t *)mem_acquire(dev, bytes, false) : nullptr;
	if (!d) { mem_release(dev, h, bytes, true, 0, 0); return fail(ENOMEM, "blockstat_batch: job table and maps"); }
	E264BlockStatJob *jobs = (E264BlockStatJob *)h;
	uint32_t max_chunks = 1;
	size_t at = jobs_bytes;
	for (int i = 0; i < n; i++) {
		jobs[i].base = streams[i]->h_table[slots[i]];
		jobs[i].slot_bytes = streams[i]->slot_bytes[slots[i]];
		jobs[i].view = views[i];
		jobs[i].dst = d + at;
		jobs[i].k = (uint32_t)log2_block;
		jobs[i].chunks = e264_blockstat_chunks(&views[i], log2_block);
		max_chunks = std::max(max_chunks, jobs[i].chunks);
		at += e264hip_blockstat_bytes(&views[i], log2_block, nullptr);
	}
	uint64_t serial;
	hipError_t e;
	{
		std::lock_guard<std::mutex> g(dev->lock);
		hipStream_t q = dev->q[lane];
		e = hipMemcpyAsync(d, h, (size_t)n * sizeof(E264BlockStatJob), hipMemcpyHostToDevice, q);
		if (e == hipSuccess) e = e264_launch_blockstat((const E264BlockStatJob *)d, n, max_chunks, q);
		if (e == hipSuccess) e = hipMemcpyAsync(h + jobs_bytes, d + jobs_bytes, total, hipMemcpyDeviceToHost, q);
		serial = next_serial(dev, lane); // (also after an error: whatever was queued reads the two blocks until the lane has passed this point)
	}
	r = e == hipSuccess ? serial_wait(dev, serial, lane) : fail(EIO, "blockstat_batch", e);
	if (!r)
		for (int i = 0; i < n; i++)
			memcpy((uint8_t *)out + (size_t)i * pitch, h + (jobs[i].dst - d), e264hip_blockstat_bytes(&views[i], log2_block, nullptr));
	mem_release(dev, h, bytes, true, serial, lane);
	mem_release(dev, d, bytes, false, serial, lane);
	return r;
}

API int e264hip_frame_blockstat(E264Stream *s, int slot, const E264View *view, int log2_block, void *out, size_t cap)
{
	if (!s) return fail(EINVAL, "frame_blockstat: null stream");
	return e264hip_blockstat_batch(s->dev, &s, &slot, view, 1, log2_block, out, cap);
}

API int e264hip_packet_upload(E264Device *dev, const void *packet, size_t bytes, E264Packet **out)
{
	if (!dev || !out) return fail(EINVAL, "null argument");
	E264PacketInfo pi;
	int r = e264_check_header(packet, bytes, &pi);
	if (r || (r = e264_check_records(packet, {nullptr, nullptr}, &pi))) return r;
	std::vector<uint8_t> unfolded; // a packet that stays in HBM is kept as the kernels read it: a wire packet is unfolded once, here
	if (pi.area) {
		unfolded.resize(e264_expanded_bytes(packet));
		bytes = e264_expand_packet(packet, ((const E264FrameHdr *)packet)->total_bytes, unfolded.data(), unfolded.size());
		packet = unfolded.data();
		pi.area = 0;
	}
	if (set_device(dev)) return EIO;
	E264Packet *p = new (std::nothrow) E264Packet();
	if (!p) return fail(ENOMEM, "packet object");
	p->dev = dev; p->info = pi;
	if (hipMalloc((void **)&p->d_bytes, bytes) != hipSuccess) { delete p; return fail(ENOMEM, "hipMalloc packet"); }
	hipError_t e = hipMemcpy(p->d_bytes, packet, bytes, hipMemcpyHostToDevice);
	if (e != hipSuccess) { hipFree(p->d_bytes); delete p; return fail(EIO, "hipMemcpy packet", e); }
	*out = p;
	return 0;
}

API void e264hip_packet_free(E264Packet *p)
{
	if (!p) return;
	hipSetDevice(p->dev->ordinal);
	e264hip_device_sync(p->dev); // a resident packet may be named by batches of any lane (benchmarks, tests: not a decoder's path)
	hipFree(p->d_bytes);
	delete p;
}

struct E264Batch {
	E264Device *dev;
	E264Job *d_jobs;
	int n, max_mbs, max_tiles, lane;
	int n_nopred;   // the table's last n_nopred jobs are pictures without inter / PCM macroblocks
	bool pred_work; // some packet of the batch has inter / PCM macroblocks (all-intra batches skip the prediction kernel's launch)
	bool has_l1;    // some packet of the batch predicts from list 1
	std::vector<std::pair<E264Stream *, int>> writes; // (stream, destination slot) of every job
};

API int e264hip_batch_create(E264Device *dev, E264Stream *const *streams, E264Packet *const *packets, int n, E264Batch **out)
{
	if (!dev || !streams || !packets || !out || n <= 0) return fail(EINVAL, "batch_create arguments");
	if (set_device(dev)) return EIO;
	std::vector<E264Job> jobs((size_t)n);
	E264Batch acc = {};
	JobOrder order = {n};
	for (int i = 0; i < n; i++) {
		if (!packets[i] || packets[i]->dev != dev) return fail(EINVAL, "batch entry");
		const E264PacketInfo &pi = packets[i]->info;
		int r; // (the packet was vetted without a stream at upload time: its slots against THIS stream's allocations)
		if ((r = check_lane(dev, streams, i)) || (r = e264_check_slots(slots_of(streams[i]), pi)) || (r = check_once(streams, i)) || (r = ensure_scratch(streams[i], pi.n_mbs()))) return r;
		E264Job &jb = jobs[(size_t)order.slot(pi.pred_work)];
		jb.packet = packets[i]->d_bytes;
		jb.dpb = streams[i]->d_table;
		jb.dbk = streams[i]->dbk.d;
		jb.expand = nullptr; // (resident packets are version 4: e264hip_packet_upload)
		acc.max_mbs = std::max(acc.max_mbs, pi.n_mbs());
		acc.max_tiles = std::max(acc.max_tiles, e264_pred_tiles(pi.width_mbs, pi.height_mbs));
		acc.pred_work = acc.pred_work || pi.pred_work; acc.has_l1 = acc.has_l1 || pi.has_l1;
		acc.writes.emplace_back(streams[i], pi.dst_slot);
	}
	acc.dev = dev; acc.n = n; acc.lane = streams[0]->lane; acc.n_nopred = order.back;
	E264Batch *b = new (std::nothrow) E264Batch(std::move(acc));
	if (!b) return fail(ENOMEM, "batch object");
	if (hipMalloc((void **)&b->d_jobs, sizeof(E264Job) * n) != hipSuccess) { delete b; return fail(ENOMEM, "hipMalloc jobs"); }
	hipError_t e = hipMemcpy(b->d_jobs, jobs.data(), sizeof(E264Job) * n, hipMemcpyHostToDevice);
	if (e != hipSuccess) { hipFree(b->d_jobs); delete b; return fail(EIO, "hipMemcpy jobs", e); }
	*out = b;
	return 0;
}

API int e264hip_batch_submit(E264Batch *b, int mode)
{
	if (!b) return fail(EINVAL, "null batch");
	if (set_device(b->dev)) return EIO;
	for (auto &w : b->writes)
		if (w.first->lane != b->lane) return fail(EINVAL, "a stream of the batch was bound to another lane after batch_create");
	uint64_t serial = 0;
	int r = launch(b->dev, b->lane, b->d_jobs, b->max_mbs, b->max_tiles, submission(b->n, b->n_nopred, mode, b->pred_work, b->has_l1), &serial);
	if (!r) for (auto &w : b->writes) publish_serial(w.first, w.second, serial);
	return r;
}

API void e264hip_batch_free(E264Batch *b)
{
	if (!b) return;
	hipSetDevice(b->dev->ordinal);
	hipStreamSynchronize(b->dev->q[b->lane]);
	hipFree(b->d_jobs);
	delete b;
}

API int e264hip_submit_batch(E264Device *dev, E264Stream *const *streams, E264Packet *const *packets, int n, int mode)
{
	E264Batch *b = nullptr;
	int r = e264hip_batch_create(dev, streams, packets, n, &b);
	if (r) return r;
	r = e264hip_batch_submit(b, mode);
	e264hip_batch_free(b); // synchronises the lane: convenience path for tests
	return r;
}

// Host packets of MANY streams, one submission, nothing synchronous: every packet is staged through its
// stream's pinned ring and copied on the upload queue, the job table through a device-level ring, then the four
// kernels are launched on the streams' lane behind the batch's upload event.  The caller may reuse / free the host
// packets on return.
enum { HOST_PINNED = 1, HOST_TRUSTED = 2 }; // submit_host_impl's flags
static size_t round_mib_quarter(size_t need) { return (need + need / 4 + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1); } // a quarter of headroom: the pictures of a stream differ in size
static int submit_host_impl(E264Device *dev, E264Stream *const *streams, const void *const *packets, const size_t *bytes, int n, int mode, int flags)
{
	const bool pinned = flags & HOST_PINNED, trusted = flags & HOST_TRUSTED;
	static const int gather_workers = getenv("E264_GATHER_THREADS") ? atoi(getenv("E264_GATHER_THREADS")) : E264_GATHER_WORKERS;
	// Page-locked packets of a LARGE batch are gathered into the batch's staging buffer like pageable ones (host threads, ~10 GB/s each) and
	// cross PCIe as one transfer: 256 separate 1-MB copies reach 35 GB/s (36 k frames/s on the bench GOP), one 246-MB copy 54 k.
	const bool stage = !pinned || n >= 32;
	if (!dev || !streams || !packets || !bytes || n <= 0) return fail(EINVAL, "submit_batch_host arguments");
	if (set_device(dev)) return EIO;
	struct Pkt {
		E264PacketInfo info;
		size_t off, xoff;                // where it lies in the batch's staging buffer, its expansion in the batch's expansion buffer
		E264Stream::Stage *st;           // (unstaged batches) its stream's staging slot
		int rc; std::string why;         // what its check said, on a pool thread, and that thread's error text
	};
	std::vector<Pkt> pk((size_t)n);
	int r;
	for (int i = 0; i < n; i++)
		if ((r = check_lane(dev, streams, i)) || (r = check_once(streams, i))) return r;
	const int lane = streams[0]->lane;
	// headers first (cheap, serial): sizes, destination slots
	int max_mbs = 0, max_tiles = 0;
	size_t total = 0, xtotal = 0;
	for (int i = 0; i < n; i++) {
		E264PacketInfo &pi = pk[i].info;
		if ((r = e264_check_header(packets[i], bytes[i], &pi))) return r;
		pk[i].xoff = xtotal;
		xtotal += (pi.area + 255) & ~(size_t)255;
		if (!streams[i]->h_table[pi.dst_slot]) return fail(EINVAL, "destination slot not allocated");
		max_tiles = std::max(max_tiles, e264_pred_tiles(pi.width_mbs, pi.height_mbs));
		max_mbs = std::max(max_mbs, pi.n_mbs());
		pk[i].off = total;
		total += (bytes[i] + 255) & ~(size_t)255;
	}
	std::lock_guard<std::mutex> bg(dev->batch_lock); // batches of one device are serialised (their streams are disjoint per batch anyway)
	// ---- every allocation first: a failure below this block would leave copies in flight on buffers nobody guards ----
	// (the ring slot is not busy: nothing in flight reads the blocks it gives back)
	E264Device::JobRing &jr = dev->jring[dev->jring_next];
	if (jr.busy) { hipEventSynchronize(jr.done); jr.busy = false; }
	const size_t jcap = ((size_t)n + 63) & ~(size_t)63, pcap = round_mib_quarter(total), xcap = round_mib_quarter(xtotal);
	if (jr.jobs.cap < (size_t)n && (r = buf_grow(dev, jr.jobs, jcap, sizeof(E264Job) * jcap, sizeof(E264Job) * jcap, "pinned job table", "device job table"))) return r;
	if (stage && jr.pkt.cap < total && (r = buf_grow(dev, jr.pkt, pcap, pcap, pcap, "pinned batch staging", "device batch staging"))) return r;
	if (jr.xp.cap < xtotal && (r = buf_grow(dev, jr.xp, xcap, 0, xcap, nullptr, "device expansion buffer"))) return r;
	if (!jr.done && hipEventCreateWithFlags(&jr.done, E264_WAIT_EVENT) != hipSuccess) { jr.done = nullptr; return fail(EIO, "hipEventCreate"); }
	if (!jr.up && hipEventCreateWithFlags(&jr.up, hipEventDisableTiming) != hipSuccess) { jr.up = nullptr; return fail(EIO, "hipEventCreate"); }
	for (int i = 0; i < n; i++) { // per-stream buffers (HIP calls: this thread only); the rings advance only when everything is there
		if ((r = ensure_scratch(streams[i], pk[i].info.n_mbs()))) return r;
		if (!stage && !(pk[i].st = stage_prepare(streams[i], bytes[i]))) return ENOMEM;
	}
	{ // every packet on its own, in parallel: the per-macroblock walk, and -- while its lines are still in the core's cache -- the copy
	  // into the batch's staging buffer.  Nothing has been queued yet: a packet that fails leaves no trace (the ring has not advanced).
		std::lock_guard<std::mutex> pg(dev->pool_user);
		dev->pool.parallel_for(n, [&](int i) {
			Pkt &p = pk[i];
			p.rc = trusted ? e264_check_slots(slots_of(streams[i]), p.info) : e264_check_records(packets[i], slots_of(streams[i]), &p.info);
			if (p.rc) { p.why = e264_err; return; } // the message lives in the worker's thread-local buffer
			if (trusted) e264_scan_trusted(packets[i], &p.info);
			if (stage) memcpy(jr.pkt.h + p.off, packets[i], bytes[i]);
		}, trusted ? gather_workers : 0);
	}
	for (int i = 0; i < n; i++)
		if (pk[i].rc) return fail(pk[i].rc, pk[i].why.c_str());
	dev->jring_next = (dev->jring_next + 1) % E264_JOB_RING;
	if (!stage) for (int i = 0; i < n; i++) streams[i]->stage_next = (streams[i]->stage_next + 1) & 3;
	// ---- copies on the upload queue, kernels on the lane behind the batch's upload event ----
	hipStream_t q = dev->q[lane], up = dev->upload_queue && dev->qup ? dev->qup : q;
	hipError_t e = hipSuccess;
	E264Job *h_jobs = (E264Job *)jr.jobs.h, *d_jobs = (E264Job *)jr.jobs.d;
	JobOrder order = {n};
	bool batch_l1 = false;
	for (int i = 0; i < n; i++) {
		E264Job &jb = h_jobs[order.slot(pk[i].info.pred_work)];
		jb.packet = stage ? jr.pkt.d + pk[i].off : pk[i].st->d;
		jb.dpb = streams[i]->d_table; jb.dbk = streams[i]->dbk.d;
		jb.expand = pk[i].info.area ? jr.xp.d + pk[i].xoff : nullptr;
		batch_l1 = batch_l1 || pk[i].info.has_l1;
	}
	if (!stage)
		for (int i = 0; i < n && e == hipSuccess; i++)
			e = hipMemcpyAsync(pk[i].st->d, packets[i], bytes[i], hipMemcpyHostToDevice, up);
	else
		e = hipMemcpyAsync(jr.pkt.d, jr.pkt.h, total, hipMemcpyHostToDevice, up);
	if (e == hipSuccess) e = hipMemcpyAsync(d_jobs, h_jobs, sizeof(E264Job) * n, hipMemcpyHostToDevice, up);
	if (e == hipSuccess && xtotal) { // (some packet is a wire packet)
		e = e264_launch_expand(d_jobs, n, max_mbs, up);
		if (e == hipSuccess) { std::lock_guard<std::mutex> g(dev->lock); dev->launch_counts[E264_LC_EXPAND] += (uint64_t)n; }
	}
	if (e == hipSuccess && up != q) {
		e = hipEventRecord(jr.up, up);
		if (e == hipSuccess) e = hipStreamWaitEvent(q, jr.up, 0);
	}
	uint64_t serial = 0;
	r = e == hipSuccess ? launch(dev, lane, d_jobs, max_mbs, max_tiles, submission(n, order.back, mode, order.back != n, batch_l1), &serial) : fail(EIO, "packet upload", e);
	if (r && up != q) hipStreamSynchronize(up); // copies already queued must not outlive the error return unguarded
	// the job table and the staging slots are busy until the lane has passed this point -- also on an error above: whatever
	// part of the batch was queued still reads them
	hipEventRecord(jr.done, q);
	jr.busy = true;
	if (!stage)
		for (int i = 0; i < n; i++) {
			hipEventRecord(pk[i].st->done, q);
			pk[i].st->busy = true;
		}
	if (r) return r;
	for (int i = 0; i < n; i++) publish_serial(streams[i], pk[i].info.dst_slot, serial);
	return 0;
}

API int e264hip_submit_batch_host(E264Device *dev, E264Stream *const *streams, const void *const *packets, const size_t *bytes, int n, int mode)
{
	return submit_host_impl(dev, streams, packets, bytes, n, mode, 0);
}
// The same for packets that already sit in page-locked memory (e264hip_host_alloc; what a front end does when it assembles
// the packet in place): no staging copy, the H2D reads the caller's buffer, which must stay untouched until the submission
// has retired (e264hip_device_sync / a later e264hip_frame_wait).  E264_SUBMIT_TRUSTED: the caller has run
// e264hip_packet_check on exactly these bytes (a packet produced by its own emitter, a validated capture): the
// per-macroblock walk is not repeated on the submitting thread; the slots the vetted header names (dst_slot, ref_slots)
// are still checked against this stream's allocations.
API int e264hip_submit_batch_pinned(E264Device *dev, E264Stream *const *streams, const void *const *packets, const size_t *bytes, int n, int mode, int flags)
{
	return submit_host_impl(dev, streams, packets, bytes, n, mode, HOST_PINNED | (flags & E264_SUBMIT_TRUSTED ? HOST_TRUSTED : 0));
}
API void *e264hip_host_alloc(E264Device *dev, size_t bytes)
{
	void *p = nullptr;
	if (!dev || set_device(dev) || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { fail(ENOMEM, "hipHostMalloc"); return nullptr; }
	return p;
}
API void e264hip_host_free(E264Device *dev, void *p)
{
	if (dev && p && !set_device(dev)) hipHostFree(p);
}

// Timing events are recorded on lane 0 AFTER everything queued on the other lanes so far (lane 0 waits for them): with one
// lane in use that is the plain event on the queue of the kernels, with several it brackets all of them.
API int e264hip_launch_counts(E264Device *dev, uint64_t *out, int n, int reset)
{
	if (!dev || (n > 0 && !out)) { fail(EINVAL, "launch_counts arguments"); return -1; }
	std::lock_guard<std::mutex> g(dev->lock);
	for (int i = 0; i < n && i < E264_LC_COUNT; i++) out[i] = i == E264_LC_N_CUS ? (uint64_t)dev->n_cus : dev->launch_counts[i];
	if (reset) memset(dev->launch_counts, 0, sizeof(dev->launch_counts));
	return E264_LC_COUNT;
}

API int e264hip_event_record(E264Device *dev, int idx)
{
	if (!dev || idx < 0 || idx >= 16) return fail(EINVAL, "event index");
	if (set_device(dev)) return EIO;
	for (int i = 1; i < E264Device::NQ; i++) {
		HIPCHK(hipEventRecord(dev->lane_ev[i], dev->q[i]), EIO);
		HIPCHK(hipStreamWaitEvent(dev->q[0], dev->lane_ev[i], 0), EIO);
	}
	HIPCHK(hipEventRecord(dev->ev[idx], dev->q[0]), EIO);
	return 0;
}

API int e264hip_event_elapsed_ms(E264Device *dev, int a, int b, float *ms)
{
	if (!dev || !ms || a < 0 || a >= 16 || b < 0 || b >= 16) return fail(EINVAL, "event index");
	if (set_device(dev)) return EIO;
	HIPCHK(hipEventSynchronize(dev->ev[b]), EIO);
	HIPCHK(hipEventElapsedTime(ms, dev->ev[a], dev->ev[b]), EIO);
	return 0;
}

// has everything queued before e264hip_event_record(dev, idx) left the GPU?  0 yes, EBUSY not yet (never blocks)
API int e264hip_event_query(E264Device *dev, int idx)
{
	if (!dev || idx < 0 || idx >= 16) return fail(EINVAL, "event index");
	if (set_device(dev)) return EIO;
	const hipError_t e = hipEventQuery(dev->ev[idx]);
	if (e == hipSuccess) return 0;
	if (e == hipErrorNotReady) { (void)hipGetLastError(); return EBUSY; }
	return fail(EIO, "hipEventQuery");
}

API int e264hip_kernel_timing(E264Device *dev, int enable)
{
	if (!dev) return fail(EINVAL, "null device");
	e264hip_device_sync(dev);
	dev->ktiming = enable != 0;
	dev->kev_used = 0;
	return 0;
}

API int e264hip_kernel_time_ms(E264Device *dev, double *ms4, int *launches)
{
	if (!dev || !ms4) return fail(EINVAL, "null argument");
	int r = e264hip_device_sync(dev);
	if (r) return r;
	ms4[0] = ms4[1] = ms4[2] = ms4[3] = 0;
	for (size_t i = 0; i < dev->kev_used; i++)
		for (int k = 0; k < 4; k++) {
			float ms = 0;
			const E264Device::Marks &m = dev->kev[i];
			const bool side = k == 0 && m.side; // the parameter kernel ran on the second queue: its own pair of events
			if (hipEventElapsedTime(&ms, side ? m.a[0] : m.e[k], side ? m.a[1] : m.e[k + 1]) == hipSuccess) ms4[k] += ms;
		}
	if (launches) *launches = (int)dev->kev_used;
	return 0;
}
