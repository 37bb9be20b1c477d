/*
 * acm_hip_api.cpp - device handle, memory plumbing, plan upload and launch
 * behind include/acm_hip.h.  The kernels are in acm_kernels.hip, what a plan
 * launches is decided in acm_plan_cut.cpp.
 */
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "acm_device.h"
#include "acm_hip.h"
#include "acm_plan_cut.h"

namespace {

thread_local char g_err[512] = "";

void set_err(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
}

} // namespace
/* (for the other translation units of the library: the text acmhip_last_error() returns on this thread) */
extern "C" void acmhip_set_error_text(const char *text)
{
	set_err("%s", text);
}
namespace {

int hip_fail(hipError_t e, const char *what)
{
	set_err("%s: %s", what, hipGetErrorString(e));
	return ACMHIP_ERR_HIP;
}

#define HIPTRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_fail(e_, #call); } while (0)

} // namespace

struct acmhip_device {
	int ordinal;
	hipStream_t stream;
	bool own_stream;
	hipStream_t copy_stream = nullptr;      /* read-back stream of the batch pipeline, created on first use */
	hipStream_t side[2] = { nullptr, nullptr };     /* plans with several level groups spread them over these too */
	hipStream_t upload = nullptr;           /* plan tables go up on a non-blocking stream of their own (to_device) */
	hipStream_t aux[ACM_AUX_STREAMS] = {};  /* the batch pipeline's per-group upload + bit-parsing streams, created on first use */
	std::mutex upload_mutex;
	/* pinned staging ring of the table uploads: a copy out of pinned memory returns when it is queued, so a plan waits once for all its
	 * tables (or not at all: ACMHIP_PLAN_UPLOAD_ASYNC) instead of once per table */
	uint8_t *up_ring = nullptr;
	bool up_ring_failed = false;            /* pinning the ring failed once: tables go up straight from where they are */
	size_t up_at = 0;
	static constexpr size_t UP_RING_BYTES = (size_t)32 << 20;
	int cus = 0;                            /* compute units, sizes the persistent grids */
	void *arena[ACM_ARENA_SLOTS] = {};
	size_t arena_cap[ACM_ARENA_SLOTS] = {};
	std::mutex arena_mutex;
	/* A call's hold on the arenas is an epoch (acmhip_arena_lock); arena_asked[slot] = the bytes the call of epoch arena_epoch_of[slot]
	 * asked of the slot: what acmhip_device_arena_info reports, and with the fill mode on (acmhip_device_set_fill) what has been filled
	 * for that call */
	bool fill = false;
	acmhip_launch_caps caps{};              /* acmhip_device_set_launch_caps: all zero = every built-in value */
	uint64_t arena_epoch = 0;
	uint64_t arena_epoch_of[ACM_ARENA_SLOTS] = {};
	size_t arena_asked[ACM_ARENA_SLOTS] = {};
	/* device blocks of destroyed plans (tile tables, planes, the lead-in sink), kept for the next plan: hipMalloc / hipFree
	 * synchronise the whole device - every stream of the process, an RCCL transfer in flight included - and a batch builds and
	 * drops a plan per chunk */
	struct Block {
		void *ptr;
		size_t bytes;
	};
	std::vector<Block> spare;
	size_t spare_bytes = 0;
	std::mutex spare_mutex;
	static constexpr size_t SPARE_MAX_BYTES = (size_t)768 << 20, SPARE_MAX_BLOCKS = 256;
};

/* per level: the fused-kernel tile table, or the stage-wise stream list */
struct LevelGroup {
	uint32_t level = 0;
	AcmTile *d_tiles = nullptr;
	uint32_t ntiles = 0;
	bool carry = false;         /* tile table cut for the carry-mode kernel (no halo rows, ACM_TILE_* flags) */
	AcmTile2 *d_tiles2 = nullptr;   /* whole tiles of streams decoded from row 0: the lean kernel (acm_tile2) */
	uint32_t ntiles2 = 0;
	/* the whole tiles of the streams that came with a packed form: as records of the packed build (acm_tile2p; idx_off = packed tile
	 * number) and as plain acm_tile2 records over the int16 arena, which a launch uses while no packed arenas are bound */
	AcmTile2 *d_tiles2p = nullptr, *d_tiles2p_plain = nullptr;
	uint32_t ntiles2p = 0;
	/* the same for streams that came with a byte-plane form (acm_tile2's matrix-core build) */
	AcmTile2 *d_tiles2m = nullptr, *d_tiles2m_plain = nullptr;
	uint32_t ntiles2m = 0, ntiles2m_plain = 0;      /* the matrix-core build may cut the same rows into smaller tiles */
	uint32_t *d_claim = nullptr;                    /* the chunk kernel's claim word for d_tiles2m (acmk_launch_tile2m): zero between launches */
	AcmTile *d_tiles_extra = nullptr;   /* halo-flavour tiles that must not join a carry run (clean tiles of patched streams) */
	uint32_t ntiles_extra = 0;
	uint32_t *d_list = nullptr;
	uint32_t nlist = 0;
	uint64_t max_elems = 0;     /* stage-wise: longest plane run in the group */
	uint64_t max_emit = 0;
	bool prefix_patched = false;    /* a stream of the group has H1 patches: unpack, patch and stage 0 stay separate launches */
	uint32_t prefix_stages = 0; /* levels 13-15: the stage-wise kernels do level - 12 stages, the level-12 plane kernel the rest (d_tiles) */
};

struct acmhip_plan {
	acmhip_device *dev = nullptr;
	std::vector<acmhip_device::Block> blocks;       /* every device allocation of this plan (handed back to the handle's spare list) */
	AcmDevStream *d_streams = nullptr;
	std::vector<LevelGroup> fused, stagewise, small, prefix;   /* small: levels 0-4, one register-cascade launch; prefix: levels 13-15 */
	int16_t *d_sink = nullptr;             /* acm_tile2: where lead-in tiles store the PCM nobody wants */
	std::vector<uint64_t> form_rows;       /* per stream: rows the plan reads from the stream's second staged form (acmhip_plan_form_rows) */
	uint32_t *d_sw_all = nullptr;          /* every stage-wise stream, for the unpack launch */
	uint32_t n_sw_all = 0;
	uint64_t sw_max_elems = 0;
	AcmDevPatch *d_patches = nullptr;
	uint64_t npatches = 0;
	int32_t *d_plane[2] = { nullptr, nullptr };
	uint64_t plane_elems = 0;
	acmhip_plan_stats stats{};
	const acmhip_packed_chunk *pk_chunks = nullptr; /* acmhip_plan_bind_packed: device tables of the packed staged form */
	const uint8_t *pk_blob = nullptr;
	const uint8_t *mform = nullptr;                 /* acmhip_plan_bind_mform */
	const acmhip_mform_pair *mform_pairs = nullptr;
	int variant = 0;                        /* fused-kernel variant the tile tables were cut for */
	/* several tile-kernel groups (a corpus of mixed levels): their launches are independent, so they go round robin
	 * over the device stream and two side streams - the ramp-up and the tail of one launch overlap the next one's
	 * instead of leaving the chip half empty three times (fork / join by events on the device stream) */
	hipEvent_t ev_fork = nullptr, ev_join[2] = { nullptr, nullptr };
	hipEvent_t ev_upload = nullptr;         /* ACMHIP_PLAN_UPLOAD_ASYNC: the tables are on the device once this has happened */
	bool tables_settled = false;            /* upload_done() has run: waited for, or covered by ev_upload */
	bool form_only = false;                 /* ACMHIP_PLAN_FORM_ONLY: no int16 twin of the byte-plane records */
};

extern "C" const char *acmhip_last_error(void)
{
	return g_err;
}

extern "C" int acmhip_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) {
		(void)hipGetLastError();
		return 0;
	}
	return n;
}

extern "C" int acmhip_device_open(int ordinal, void *hip_stream, acmhip_device **out)
{
	if (!out)
		return ACMHIP_ERR_ARG;
	/* a library whose kernels and whose planner were compiled with different -D flags (profiles/build_variant.sh) would cut tables for
	 * other tiles than its kernels walk */
	if (acmk_geo_digest() != acmk_geo_digest_kernels()) {
		set_err("mixed build: the kernels were compiled for another launch geometry than the planner (acm_kernel_geo.h digest %016llx, kernels %016llx)",
			(unsigned long long)acmk_geo_digest(), (unsigned long long)acmk_geo_digest_kernels());
		return ACMHIP_ERR_ARG;
	}
	int n = acmhip_device_count();
	if (n <= 0) {
		set_err("no usable HIP device (hipGetDeviceCount found none); this library has no CPU synthesis path");
		return ACMHIP_ERR_NO_DEVICE;
	}
	if (ordinal < 0 || ordinal >= n) {
		set_err("device ordinal %d out of range (have %d)", ordinal, n);
		return ACMHIP_ERR_ARG;
	}
	HIPTRY(hipSetDevice(ordinal));
	acmhip_device *d = new (std::nothrow) acmhip_device;
	if (!d)
		return ACMHIP_ERR_NOMEM;
	d->ordinal = ordinal;
	{
		hipDeviceProp_t prop;
		if (hipGetDeviceProperties(&prop, ordinal) == hipSuccess)
			d->cus = prop.multiProcessorCount;
	}
	d->own_stream = (hip_stream == nullptr);
	d->stream = (hipStream_t)hip_stream;
	if (d->own_stream) {
		hipError_t e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
		if (e != hipSuccess) {
			delete d;
			return hip_fail(e, "hipStreamCreateWithFlags");
		}
	}
	/* the streams of the batch pipeline that run concurrently - kernels (above), read-back, upload - are created here, one
	 * after the other: the runtime hands out its few hardware queues in creation order, so these three get one each as long
	 * as queues are left (created later, between whatever else the process creates, two of them may share one, and an
	 * upload then waits behind every read-back).  Failing here is not fatal: they are created on first use otherwise */
	if (hipStreamCreateWithFlags(&d->copy_stream, hipStreamNonBlocking) != hipSuccess)
		d->copy_stream = nullptr;
	if (hipStreamCreateWithFlags(&d->aux[ACM_AUX_STREAMS - 1], hipStreamNonBlocking) != hipSuccess)
		d->aux[ACM_AUX_STREAMS - 1] = nullptr;
	(void)hipGetLastError();
	*out = d;
	return ACMHIP_OK;
}

extern "C" void acmhip_device_close(acmhip_device *dev)
{
	if (!dev)
		return;
	(void)hipSetDevice(dev->ordinal);
	(void)hipStreamSynchronize(dev->stream);
	for (const acmhip_device::Block &b : dev->spare)
		(void)hipFree(b.ptr);
	for (int k = 0; k < ACM_ARENA_SLOTS; k++) {
		if (!dev->arena[k])
			continue;
		if (acm_arena_is_host(k))
			(void)hipHostFree(dev->arena[k]);
		else
			(void)hipFree(dev->arena[k]);
	}
	if (dev->copy_stream)
		(void)hipStreamDestroy(dev->copy_stream);
	if (dev->upload)
		(void)hipStreamDestroy(dev->upload);
	if (dev->up_ring)
		(void)hipHostFree(dev->up_ring);
	for (hipStream_t s : dev->aux)
		if (s)
			(void)hipStreamDestroy(s);
	for (hipStream_t s : dev->side)
		if (s)
			(void)hipStreamDestroy(s);
	if (dev->own_stream)
		(void)hipStreamDestroy(dev->stream);
	delete dev;
}

namespace {

const char *const g_slot_names[ACM_ARENA_SLOTS] = {
	"H_IDX", "H_HDR", "H_PCM", "H_FILES", "H_JOBS", "H_PKBLOB", "H_PKCHUNK",
	"D_IDX", "D_HDR", "D_PCM", "D_FILES", "D_COLPOS", "D_JOBS", "D_STAGE",
	"D_PKBLOB", "D_PKCHUNK", "D_BLKOFF", "D_MARKS", "H_MARKS", "D_SRC", "D_FEAT",
};

/* What the fill mode leaves in a slot (acmhip_device_set_fill):
 *   D_PCM, H_PCM, D_SRC, D_FEAT   0xA5 - output only (D_FEAT holds the rows a features call frames, and behind them the DFT operand its own launch writes in full; D_SRC holds the PCM rows an overlay call combines: a row nobody wrote is visibly wrong): nothing reads a sample back, and the pattern is the one the arena-contract tests poison with;
 *   D_IDX, H_IDX   0x5A (index 0x5A5A) - the staged int16 indices are operands and nothing else: the parser's column kernel and the host
 *                  stagers only store them, the synthesis kernels multiply them by the block's val (value = idx * val) and the packers
 *                  compare them with class bounds; no kernel forms an address, an LDS offset or a trip count from one, so a row nobody
 *                  staged decodes to PCM that is visibly wrong instead of to silence;
 *   the rest       zero.  The file and stage arenas feed the bit reader, whose codes become column lengths and loop bounds, and the
 *                  readers count on zeros behind a file where a stripe or a slot ends; jobs, results and flags, colpos, blkoff, the
 *                  pair tables and chunk tables, the blobs (their first bytes name LDS places) and the marks are offsets, classes and
 *                  bounds, and they are read past what a call wrote (32 pair-table entries, 64 arena bytes, entries two chunks ahead):
 *                  zero is a valid place, class, offset and bound in every one of them; the headers (val, pwr) go with them */
int fill_byte(int slot)
{
	switch (slot) {
	case ACM_ARENA_D_PCM:
	case ACM_ARENA_H_PCM:
	case ACM_ARENA_D_SRC:
	case ACM_ARENA_D_FEAT:
		return 0xA5;
	case ACM_ARENA_D_IDX:
	case ACM_ARENA_H_IDX:
		return 0x5A;
	default:
		return 0;
	}
}

#define ACM_FILL_TRY(call) do { const int rc_ = (call); if (rc_ != ACMHIP_OK) return rc_; } while (0)

/* The bytes this call (epoch) has asked of the slot so far; in fill mode bytes [that, bytes) get the slot's fill first - the first
 * acmhip_arena_get of a call fills all it asks for, a second one of the same slot only what it asks beyond that (live data is never
 * wiped).  Device memory: a memset on the device stream that has ended when this returns - the streams of the call that asks are all
 * idle until then */
int note_slot(acmhip_device *dev, int slot, size_t bytes)
{
	if (dev->arena_epoch_of[slot] != dev->arena_epoch) {
		dev->arena_epoch_of[slot] = dev->arena_epoch;
		dev->arena_asked[slot] = 0;
	}
	const size_t have = dev->arena_asked[slot];
	if (bytes <= have)
		return ACMHIP_OK;
	if (dev->fill) {
		uint8_t *at = static_cast<uint8_t *>(dev->arena[slot]) + have;
		if (acm_arena_is_host(slot)) {
			memset(at, fill_byte(slot), bytes - have);
		} else {
			HIPTRY(hipSetDevice(dev->ordinal));
			HIPTRY(hipMemsetAsync(at, fill_byte(slot), bytes - have, dev->stream));
			HIPTRY(hipStreamSynchronize(dev->stream));
		}
	}
	dev->arena_asked[slot] = bytes;
	return ACMHIP_OK;
}

} // namespace

extern "C" int acmhip_device_set_fill(acmhip_device *dev, int on)
{
	if (!dev)
		return ACMHIP_ERR_ARG;
	std::lock_guard<std::mutex> g(dev->arena_mutex);
	const int was = dev->fill ? 1 : 0;
	dev->fill = on != 0;
	return was;
}

extern "C" int acmhip_device_set_launch_caps(acmhip_device *dev, const acmhip_launch_caps *caps, acmhip_launch_caps *previous)
{
	if (!dev)
		return ACMHIP_ERR_ARG;
	std::lock_guard<std::mutex> g(dev->arena_mutex);
	return acmk_launch_caps_set(&dev->caps, caps, previous);
}

extern "C" acmhip_launch_caps acmhip_device_launch_caps(const acmhip_device *dev)
{
	return dev ? dev->caps : acmhip_launch_caps{};
}

extern "C" int acmhip_device_arena_info(acmhip_device *dev, int slot, const char **name, void **ptr, size_t *bytes, int *is_host, int *fill)
{
	if (!dev || slot < 0 || slot >= ACM_ARENA_SLOTS)
		return ACMHIP_ERR_ARG;
	if (name)
		*name = g_slot_names[slot];
	if (ptr)
		*ptr = dev->arena[slot];
	if (bytes)
		*bytes = dev->arena_epoch_of[slot] == dev->arena_epoch ? dev->arena_asked[slot] : 0;
	if (is_host)
		*is_host = acm_arena_is_host(slot);
	if (fill)
		*fill = fill_byte(slot);
	return ACMHIP_OK;
}

extern "C" int acmhip_arena_get(acmhip_device *dev, int slot, size_t bytes, void **out)
{
	if (!dev || slot < 0 || slot >= ACM_ARENA_SLOTS || !out)
		return ACMHIP_ERR_ARG;
	if (bytes < 16)
		bytes = 16;
	if (dev->arena_cap[slot] < bytes) {
		HIPTRY(hipSetDevice(dev->ordinal));
		if (dev->arena[slot]) {
			HIPTRY(hipStreamSynchronize(dev->stream));
			if (acm_arena_is_host(slot))
				(void)hipHostFree(dev->arena[slot]);
			else
				(void)hipFree(dev->arena[slot]);
			dev->arena[slot] = nullptr;
			dev->arena_cap[slot] = 0;
		}
		const size_t want = bytes + bytes / 8;          /* a little headroom against creeping batches */
		if (acm_arena_is_host(slot))
			HIPTRY(hipHostMalloc(&dev->arena[slot], want, hipHostMallocDefault));
		else
			HIPTRY(hipMalloc(&dev->arena[slot], want));
		dev->arena_cap[slot] = want;
		dev->arena_asked[slot] = 0;
	}
	ACM_FILL_TRY(note_slot(dev, slot, bytes));
	*out = dev->arena[slot];
	return ACMHIP_OK;
}

extern "C" int acmhip_copy_stream(acmhip_device *dev, void **out)
{
	if (!dev || !out)
		return ACMHIP_ERR_ARG;
	HIPTRY(hipSetDevice(dev->ordinal));             /* also makes the device current for the calling thread */
	if (!dev->copy_stream)
		HIPTRY(hipStreamCreateWithFlags(&dev->copy_stream, hipStreamNonBlocking));
	*out = (void *)dev->copy_stream;
	return ACMHIP_OK;
}

extern "C" int acmhip_aux_stream(acmhip_device *dev, int k, void **out)
{
	if (!dev || !out || k < 0 || k >= ACM_AUX_STREAMS)
		return ACMHIP_ERR_ARG;
	HIPTRY(hipSetDevice(dev->ordinal));
	if (!dev->aux[k])
		HIPTRY(hipStreamCreateWithFlags(&dev->aux[k], hipStreamNonBlocking));
	*out = (void *)dev->aux[k];
	return ACMHIP_OK;
}

extern "C" int acmhip_report_hip(int hip_error, const char *what)
{
	return hip_fail((hipError_t)hip_error, what);
}

extern "C" void acmhip_arena_lock(acmhip_device *dev)
{
	if (dev) {
		dev->arena_mutex.lock();
		dev->arena_epoch++;
	}
}

extern "C" void acmhip_arena_unlock(acmhip_device *dev)
{
	if (dev)
		dev->arena_mutex.unlock();
}

extern "C" int acmhip_device_sync(acmhip_device *dev)
{
	if (!dev)
		return ACMHIP_ERR_ARG;
	HIPTRY(hipStreamSynchronize(dev->stream));
	return ACMHIP_OK;
}

extern "C" void *acmhip_device_stream(acmhip_device *dev)
{
	return dev ? (void *)dev->stream : nullptr;
}

extern "C" int acmhip_malloc(acmhip_device *dev, size_t bytes, void **dptr)
{
	if (!dev || !dptr)
		return ACMHIP_ERR_ARG;
	HIPTRY(hipSetDevice(dev->ordinal));
	HIPTRY(hipMalloc(dptr, bytes ? bytes : 16));
	return ACMHIP_OK;
}

extern "C" int acmhip_free(acmhip_device *dev, void *dptr)
{
	if (!dev)
		return ACMHIP_ERR_ARG;
	if (dptr)
		HIPTRY(hipFree(dptr));
	return ACMHIP_OK;
}

extern "C" int acmhip_host_alloc(size_t bytes, void **hptr)
{
	if (!hptr)
		return ACMHIP_ERR_ARG;
	if (acmhip_device_count() <= 0) {
		set_err("no usable HIP device: cannot allocate pinned host memory");
		return ACMHIP_ERR_NO_DEVICE;
	}
	HIPTRY(hipHostMalloc(hptr, bytes ? bytes : 16, hipHostMallocDefault));
	return ACMHIP_OK;
}

extern "C" int acmhip_host_free(void *hptr)
{
	if (hptr)
		HIPTRY(hipHostFree(hptr));
	return ACMHIP_OK;
}

extern "C" int acmhip_upload(acmhip_device *dev, void *dptr, const void *hptr, size_t bytes)
{
	if (!dev)
		return ACMHIP_ERR_ARG;
	if (bytes)
		HIPTRY(hipMemcpyAsync(dptr, hptr, bytes, hipMemcpyHostToDevice, dev->stream));
	return ACMHIP_OK;
}

extern "C" int acmhip_download(acmhip_device *dev, void *hptr, const void *dptr, size_t bytes)
{
	if (!dev)
		return ACMHIP_ERR_ARG;
	if (bytes)
		HIPTRY(hipMemcpyAsync(hptr, dptr, bytes, hipMemcpyDeviceToHost, dev->stream));
	return ACMHIP_OK;
}

extern "C" int acmhip_memset(acmhip_device *dev, void *dptr, int byte, size_t bytes)
{
	if (!dev)
		return ACMHIP_ERR_ARG;
	if (bytes)
		HIPTRY(hipMemsetAsync(dptr, byte, bytes, dev->stream));
	return ACMHIP_OK;
}

/* ------------------------------------------------------------------------ */

namespace {

/* fill mode: a block on its way into a plan - one a destroyed plan handed back (idle: acmhip_plan_destroy waits for its plan's
 * launches and uploads first), or a fresh one - is zeroed on the upload stream, in front of the tables that are queued there next; a
 * plan's launches wait for that stream (upload_done).  Tables, stream lists, planes and the sink hold offsets, places and bounds: zero
 * is a valid one everywhere.  Blocks of live plans are not on the spare list and are never touched */
int fill_block(acmhip_device *dev, void *p, size_t bytes)
{
	std::lock_guard<std::mutex> g(dev->upload_mutex);
	if (!dev->upload)
		HIPTRY(hipStreamCreateWithFlags(&dev->upload, hipStreamNonBlocking));
	HIPTRY(hipMemsetAsync(p, 0, bytes, dev->upload));
	return ACMHIP_OK;
}

/* device memory for a plan: a spare block of a destroyed plan if one fits (no more than twice the size), else hipMalloc */
int plan_malloc(acmhip_plan *pl, void **out, size_t bytes)
{
	acmhip_device *dev = pl->dev;
	*out = nullptr;
	if (bytes < 256)
		bytes = 256;
	{
		std::lock_guard<std::mutex> g(dev->spare_mutex);
		size_t best = dev->spare.size();
		for (size_t k = 0; k < dev->spare.size(); k++)
			if (dev->spare[k].bytes >= bytes && dev->spare[k].bytes <= 2 * bytes + 4096 &&
			    (best == dev->spare.size() || dev->spare[k].bytes < dev->spare[best].bytes))
				best = k;
		if (best != dev->spare.size()) {
			const acmhip_device::Block b = dev->spare[best];
			dev->spare.erase(dev->spare.begin() + (long)best);
			dev->spare_bytes -= b.bytes;
			pl->blocks.push_back(b);
			*out = b.ptr;
			return dev->fill ? fill_block(dev, b.ptr, b.bytes) : ACMHIP_OK;
		}
	}
	void *p = nullptr;
	HIPTRY(hipMalloc(&p, bytes));
	pl->blocks.push_back(acmhip_device::Block{ p, bytes });
	*out = p;
	return dev->fill ? fill_block(dev, p, bytes) : ACMHIP_OK;
}

template <typename T>
int to_device(acmhip_plan *pl, const std::vector<T> &v, T **out)
{
	acmhip_device *dev = pl->dev;
	*out = nullptr;
	if (v.empty())
		return ACMHIP_OK;
	{
		const int rc = plan_malloc(pl, (void **)out, v.size() * sizeof(T));
		if (rc != ACMHIP_OK)
			return rc;
	}
	/* on a non-blocking stream of the handle's own: neither the device stream - which may be the caller's and busy with the chunks of a
	 * batch still in flight (acm_batch_decode builds the plan of chunk k+1 while chunk k runs) - nor the legacy null stream, whose copies
	 * join every blocking stream of the process and are refused while another thread captures a graph, is involved.  The table goes
	 * through the pinned ring (the host vector dies with the caller) and is on the device when upload_done() has returned */
	const size_t bytes = (v.size() * sizeof(T) + 255) & ~(size_t)255;
	std::lock_guard<std::mutex> g(dev->upload_mutex);
	if (!dev->upload)
		HIPTRY(hipStreamCreateWithFlags(&dev->upload, hipStreamNonBlocking));
	/* (the ring is pinned when the first table of 256 KB or more comes by: a handle that only ever decodes a file or two - acmtool -d -
	 * does not pay for 32 MB of pinned memory, its few small tables go up straight from where they are) */
	if (!dev->up_ring && !dev->up_ring_failed && bytes >= ((size_t)256 << 10) && bytes <= acmhip_device::UP_RING_BYTES) {
		/* (no pinned memory to be had is not a reason to fail the plan: "no ring", the direct copy below does the same job - ADVICE r5) */
		if (hipHostMalloc((void **)&dev->up_ring, acmhip_device::UP_RING_BYTES, hipHostMallocDefault) != hipSuccess) {
			(void)hipGetLastError();
			dev->up_ring = nullptr;
			dev->up_ring_failed = true;
		}
	}
	if (!dev->up_ring || bytes > acmhip_device::UP_RING_BYTES) {
		HIPTRY(hipMemcpyAsync(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, dev->upload));
		HIPTRY(hipStreamSynchronize(dev->upload));
		return ACMHIP_OK;
	}
	if (dev->up_at + bytes > acmhip_device::UP_RING_BYTES) {
		HIPTRY(hipStreamSynchronize(dev->upload));     /* the ring is free again once everything queued from it has gone */
		dev->up_at = 0;
	}
	memcpy(dev->up_ring + dev->up_at, v.data(), v.size() * sizeof(T));
	HIPTRY(hipMemcpyAsync(*out, dev->up_ring + dev->up_at, v.size() * sizeof(T), hipMemcpyHostToDevice, dev->upload));
	dev->up_at += bytes;
	return ACMHIP_OK;
}

/* the tables of a new plan are on the device: waited for here, or (async) left to an event the plan's launches wait for */
int upload_done(acmhip_plan *pl, bool async)
{
	acmhip_device *dev = pl->dev;
	std::lock_guard<std::mutex> g(dev->upload_mutex);
	if (!dev->upload) {
		pl->tables_settled = true;
		return ACMHIP_OK;
	}
	if (!async) {
		HIPTRY(hipStreamSynchronize(dev->upload));
		pl->tables_settled = true;
		return ACMHIP_OK;
	}
	HIPTRY(hipEventCreateWithFlags(&pl->ev_upload, hipEventDisableTiming));
	HIPTRY(hipEventRecord(pl->ev_upload, dev->upload));
	pl->tables_settled = true;
	return ACMHIP_OK;
}

/* the tables of one group go up from where the cutter left them */
int upload_group(acmhip_plan *pl, const AcmCutGroup &c, LevelGroup *g)
{
	g->level = c.level;
	g->carry = c.carry;
	g->max_elems = c.max_elems;
	g->max_emit = c.max_emit;
	g->prefix_patched = c.prefix_patched;
	g->prefix_stages = c.prefix_stages;
	g->ntiles = (uint32_t)c.tiles.size();
	g->ntiles_extra = (uint32_t)c.tiles_extra.size();
	g->ntiles2 = (uint32_t)c.tiles2.size();
	g->ntiles2p = (uint32_t)c.tiles2p.size();
	g->ntiles2m = (uint32_t)c.tiles2m.size();
	g->ntiles2m_plain = (uint32_t)c.tiles2m_plain.size();
	g->nlist = (uint32_t)c.list.size();
	int rc = ACMHIP_OK;
	auto up = [&](const auto &v, auto **d) {
		if (rc == ACMHIP_OK)
			rc = to_device(pl, v, d);
	};
	up(c.tiles, &g->d_tiles);
	up(c.tiles_extra, &g->d_tiles_extra);
	up(c.tiles2, &g->d_tiles2);
	up(c.tiles2p, &g->d_tiles2p);
	up(c.tiles2p_plain, &g->d_tiles2p_plain);
	up(c.tiles2m, &g->d_tiles2m);
	up(c.tiles2m_plain, &g->d_tiles2m_plain);
	up(c.list, &g->d_list);
	/* the word in which the chunk kernel's wavefronts count the runs they claim: one per group is enough, a plan's launches follow each
	 * other on the device's one stream.  Zeroed once, on the upload stream with the tables; every launch leaves it at zero */
	if (rc == ACMHIP_OK && g->ntiles2m && acmk_tile2m_run_waves(g->level, pl->dev->cus) > 0) {
		rc = plan_malloc(pl, (void **)&g->d_claim, 256);
		if (rc == ACMHIP_OK && !pl->dev->fill)
			rc = fill_block(pl->dev, g->d_claim, 256);
	}
	return rc;
}

int upload_groups(acmhip_plan *pl, const std::vector<AcmCutGroup> &from, std::vector<LevelGroup> *to)
{
	int rc = ACMHIP_OK;
	for (size_t k = 0; k < from.size() && rc == ACMHIP_OK; k++) {
		to->emplace_back();
		rc = upload_group(pl, from[k], &to->back());
	}
	return rc;
}

} // namespace

extern "C" void acmhip_plan_destroy(acmhip_plan *plan)
{
	if (!plan)
		return;
	if (plan->dev) {
		(void)hipSetDevice(plan->dev->ordinal);
		(void)hipStreamSynchronize(plan->dev->stream);   /* the launches of this plan are done with its tables (side streams join the device stream) */
		if (!plan->tables_settled && plan->dev->upload) {
			/* a plan whose creation failed half way has tables queued on the upload stream and no event that says when they have gone:
			 * wait for the stream itself before its blocks are handed on or freed */
			std::lock_guard<std::mutex> g(plan->dev->upload_mutex);
			(void)hipStreamSynchronize(plan->dev->upload);
		}
	}
	if (plan->ev_upload) {
		(void)hipEventSynchronize(plan->ev_upload);      /* (a plan dropped before it was launched: its blocks may be handed on) */
		(void)hipEventDestroy(plan->ev_upload);
	}
	if (plan->ev_fork)
		(void)hipEventDestroy(plan->ev_fork);
	for (hipEvent_t e : plan->ev_join)
		if (e)
			(void)hipEventDestroy(e);
	if (plan->dev) {
		acmhip_device *dev = plan->dev;
		std::vector<acmhip_device::Block> drop;
		{
			std::lock_guard<std::mutex> g(dev->spare_mutex);
			for (const acmhip_device::Block &b : plan->blocks) {
				if (dev->spare.size() < acmhip_device::SPARE_MAX_BLOCKS && dev->spare_bytes + b.bytes <= acmhip_device::SPARE_MAX_BYTES &&
				    b.bytes <= acmhip_device::SPARE_MAX_BYTES / 4) {
					dev->spare.push_back(b);
					dev->spare_bytes += b.bytes;
				} else {
					drop.push_back(b);
				}
			}
		}
		for (const acmhip_device::Block &b : drop)
			(void)hipFree(b.ptr);
	}
	delete plan;
}

extern "C" int acmhip_plan_create(acmhip_device *dev, const acmhip_stream_desc *streams, size_t n,
				  const acmhip_patch *patches, size_t npatches, unsigned flags,
				  acmhip_plan **out)
{
	return acmhip_plan_create_packed(dev, streams, n, nullptr, patches, npatches, flags, out);
}

extern "C" int acmhip_plan_create_packed(acmhip_device *dev, const acmhip_stream_desc *streams, size_t n, const acmhip_packed_stream *packed,
					 const acmhip_patch *patches, size_t npatches, unsigned flags, acmhip_plan **out)
{
	if (!dev || !out || (n && !streams) || (npatches && !patches) || n > 0xFFFFFFFFull)
		return ACMHIP_ERR_ARG;
	HIPTRY(hipSetDevice(dev->ordinal));
	/* what to launch is decided on the host (acm_plan_cut.cpp); the rest of this function puts it on the device */
	AcmPlanCut cut;
	int rc = acm_plan_cut(dev->cus, streams, n, packed, patches, npatches, flags, &cut);
	if (rc != ACMHIP_OK)
		return rc;

	acmhip_plan *pl = new (std::nothrow) acmhip_plan;
	if (!pl)
		return ACMHIP_ERR_NOMEM;
	pl->dev = dev;
	pl->variant = cut.variant;
	pl->form_only = cut.form_only;
	pl->form_rows = std::move(cut.form_rows);
	pl->stats = cut.stats;
	rc = to_device(pl, cut.streams, &pl->d_streams);
	if (rc == ACMHIP_OK)
		rc = upload_groups(pl, cut.fused, &pl->fused);
	if (rc == ACMHIP_OK)
		rc = upload_groups(pl, cut.small, &pl->small);
	if (rc == ACMHIP_OK)
		rc = upload_groups(pl, cut.prefix, &pl->prefix);
	if (rc == ACMHIP_OK)
		rc = upload_groups(pl, cut.stagewise, &pl->stagewise);
	if (rc == ACMHIP_OK && cut.need_sink)
		rc = plan_malloc(pl, (void **)&pl->d_sink, ACM_K2_SINK_F32_BYTES);      /* (a float32 launch stores twice the bytes) */
	if (rc == ACMHIP_OK && cut.plane_elems > 0) {
		pl->n_sw_all = (uint32_t)cut.sw_all.size();
		pl->sw_max_elems = cut.sw_max_elems;
		pl->plane_elems = cut.plane_elems;
		pl->npatches = cut.patches.size();
		rc = to_device(pl, cut.sw_all, &pl->d_sw_all);
		if (rc == ACMHIP_OK)
			rc = to_device(pl, cut.patches, &pl->d_patches);
		for (int b = 0; b < 2 && rc == ACMHIP_OK; b++)
			rc = plan_malloc(pl, (void **)&pl->d_plane[b], cut.plane_elems * sizeof(int32_t));
	}
	if (rc == ACMHIP_OK)
		rc = upload_done(pl, (flags & ACMHIP_PLAN_UPLOAD_ASYNC) != 0);
	if (rc != ACMHIP_OK) {
		acmhip_plan_destroy(pl);
		return rc;
	}
	if (pl->fused.size() > 1 && !(ACM_TUNING_ENV("ACM_PLAN_STREAMS") && atoi(ACM_TUNING_ENV("ACM_PLAN_STREAMS")) <= 1)) {
		hipError_t e = hipEventCreateWithFlags(&pl->ev_fork, hipEventDisableTiming);
		for (int k = 0; k < 2 && e == hipSuccess; k++) {
			e = hipEventCreateWithFlags(&pl->ev_join[k], hipEventDisableTiming);
			if (e == hipSuccess && !dev->side[k])
				e = hipStreamCreateWithFlags(&dev->side[k], hipStreamNonBlocking);
		}
		if (e != hipSuccess) {
			rc = hip_fail(e, "side streams of a multi-level plan");
			acmhip_plan_destroy(pl);
			return rc;
		}
	}
	*out = pl;
	return ACMHIP_OK;
}

extern "C" int acmhip_plan_form_rows(const acmhip_plan *plan, size_t stream, uint64_t *rows)
{
	if (!plan || !rows || stream >= plan->form_rows.size())
		return ACMHIP_ERR_ARG;
	*rows = plan->form_rows[stream];
	return ACMHIP_OK;
}

extern "C" int acmhip_plan_get_stats(const acmhip_plan *plan, acmhip_plan_stats *out)
{
	if (!plan || !out)
		return ACMHIP_ERR_ARG;
	*out = plan->stats;
	return ACMHIP_OK;
}

#define LAUNCHTRY(call) do { int e_ = (call); if (e_ != 0) { \
	if (e_ > 0) return hip_fail((hipError_t)e_, #call); \
	set_err("%s: unsupported configuration", #call); return ACMHIP_ERR_ARG; } } while (0)

/* fmt: ACMHIP_FMT_*, or ACMK_FMT_F32 for float32 samples (d_pcm then holds floats) */
static int plan_launch(acmhip_plan *pl, const int16_t *d_idx, const acmhip_blkhdr *d_hdr, int16_t *d_pcm, unsigned fmt)
{
	void *st = (void *)pl->dev->stream;
	if (pl->ev_upload)
		HIPTRY(hipStreamWaitEvent(pl->dev->stream, pl->ev_upload, 0));
	if (pl->form_only && !pl->mform)
		for (const LevelGroup &g : pl->fused)
			if (g.ntiles2m) {
				set_err("a plan cut with ACMHIP_PLAN_FORM_ONLY is launched without its byte-plane form bound");
				return ACMHIP_ERR_ARG;
			}

	const acmhip_launch_caps caps = acmhip_device_launch_caps(pl->dev);    /* plain values from here on: nothing below asks the runtime */
	const bool spread = pl->ev_fork != nullptr;
	if (spread) {
		HIPTRY(hipEventRecord(pl->ev_fork, pl->dev->stream));
		for (int k = 0; k < 2; k++)
			HIPTRY(hipStreamWaitEvent(pl->dev->side[k], pl->ev_fork, 0));
	}
	/* The lean kernels of every level group, ONE BEHIND THE OTHER on the device stream: each of them fills the chip by itself (the planner
	 * hands a level's tiles to them only from eight per workgroup on), and the chunk kernel's workgroup IS a CU - two of them overlapping
	 * on separate streams share the CUs between them and both run at half rate until the shorter one ends, with whatever comes third
	 * waiting for a whole CU's LDS (the configs[2] corpus, levels 7-9 in one plan: 1.78 ms a step with the groups spread over three
	 * streams, round 6).  What IS spread over the side streams are the small kernels behind them - the ragged tails on acm_fused_tile -
	 * which fill the gaps the big ones leave */
	for (const LevelGroup &g : pl->fused) {
		LAUNCHTRY(acmk_launch_tile2(g.level, pl->dev->cus, g.d_tiles2, g.ntiles2, d_idx, d_hdr, d_pcm, pl->d_sink, fmt, st));
		if (pl->pk_chunks)
			LAUNCHTRY(acmk_launch_tile2p(g.level, pl->dev->cus, g.d_tiles2p, g.ntiles2p, pl->pk_chunks, pl->pk_blob, d_hdr, d_pcm, pl->d_sink, fmt, st));
		else
			LAUNCHTRY(acmk_launch_tile2(g.level, pl->dev->cus, g.d_tiles2p_plain, g.ntiles2p, d_idx, d_hdr, d_pcm, pl->d_sink, fmt, st));
		if (pl->mform)
			LAUNCHTRY(acmk_launch_tile2m(g.level, pl->dev->cus, g.d_tiles2m, g.ntiles2m, pl->mform, pl->mform_pairs, d_hdr, d_pcm, pl->d_sink, fmt, g.d_claim, st));
		else
			LAUNCHTRY(acmk_launch_tile2(g.level, pl->dev->cus, g.d_tiles2m_plain, g.ntiles2m_plain, d_idx, d_hdr, d_pcm, pl->d_sink, fmt, st));
	}
	size_t gi = 0;
	for (const LevelGroup &g : pl->fused) {
		void *gs = (!spread || gi % 3 == 0) ? st : (void *)pl->dev->side[gi % 3 - 1];
		gi++;
		LAUNCHTRY(acmk_launch_fused(g.level, pl->variant, pl->dev->cus, g.carry, pl->d_streams, g.d_tiles, g.ntiles, d_idx, d_hdr, d_pcm, fmt, gs));
		LAUNCHTRY(acmk_launch_fused(g.level, pl->variant, pl->dev->cus, 0, pl->d_streams, g.d_tiles_extra, g.ntiles_extra, d_idx, d_hdr, d_pcm, fmt, gs));
	}
	if (spread) {
		for (int k = 0; k < 2; k++) {
			HIPTRY(hipEventRecord(pl->ev_join[k], pl->dev->side[k]));
			HIPTRY(hipStreamWaitEvent(pl->dev->stream, pl->ev_join[k], 0));
		}
	}

	for (const LevelGroup &g : pl->small)
		LAUNCHTRY(acmk_launch_small(g.level, pl->d_streams, g.d_list, g.nlist, g.max_emit, d_idx, d_hdr, d_pcm, fmt, caps.list_slice, caps.small_grid_x, st));

	if (pl->n_sw_all || !pl->prefix.empty()) {
		if (pl->n_sw_all)
			LAUNCHTRY(acmk_launch_unpack(pl->d_streams, pl->d_sw_all, pl->n_sw_all, pl->sw_max_elems,
						     d_idx, d_hdr, pl->d_plane[0], 0, caps.list_slice, st));
		for (const LevelGroup &g : pl->prefix)
			if (g.prefix_patched)
				LAUNCHTRY(acmk_launch_unpack(pl->d_streams, g.d_list, g.nlist, g.max_elems, d_idx, d_hdr, pl->d_plane[0], 16 - g.level, caps.list_slice, st));
		LAUNCHTRY(acmk_launch_patch(pl->d_patches, pl->npatches, pl->d_plane[0], st));
		for (const LevelGroup &g : pl->stagewise) {
			int cur = 0;
			for (uint32_t k = 0; k < g.level; k++, cur ^= 1)
				LAUNCHTRY(acmk_launch_stage(pl->d_streams, g.d_list, g.nlist, g.max_elems, g.level, k,
							    pl->d_plane[cur], pl->d_plane[cur ^ 1], 0, caps.list_slice, st));
			LAUNCHTRY(acmk_launch_emit(pl->d_streams, g.d_list, g.nlist, g.max_emit, pl->d_plane[cur],
						   d_pcm, fmt, caps.list_slice, st));
		}
		for (const LevelGroup &g : pl->prefix) {
			int cur = 0;
			if (!g.prefix_patched) {
				/* unpack and all level - 12 stages in one sweep, straight into the plane the tile kernel reads */
				LAUNCHTRY(acmk_launch_prefix(pl->d_streams, g.d_list, g.nlist, g.max_elems, g.level, d_idx, d_hdr, pl->d_plane[1], caps.list_slice, st));
				cur = 1;
			} else {
				for (uint32_t k = 0; k < g.prefix_stages; k++, cur ^= 1)
					LAUNCHTRY(acmk_launch_stage(pl->d_streams, g.d_list, g.nlist, g.max_elems, g.level, k,
								    pl->d_plane[cur], pl->d_plane[cur ^ 1], 16 - g.level, caps.list_slice, st));
			}
			LAUNCHTRY(acmk_launch_fused_plane(pl->dev->cus, g.carry, pl->d_streams, g.d_tiles, g.ntiles, pl->d_plane[cur], d_pcm, fmt, st));
		}
	}
	return ACMHIP_OK;
}

extern "C" int acmhip_plan_launch(acmhip_plan *pl, const int16_t *d_idx, const acmhip_blkhdr *d_hdr,
				  int16_t *d_pcm, unsigned fmt)
{
	if (!pl || fmt > 3)
		return ACMHIP_ERR_ARG;
	return plan_launch(pl, d_idx, d_hdr, d_pcm, fmt);
}

extern "C" int acmhip_plan_launch_f32(acmhip_plan *pl, const int16_t *d_idx, const acmhip_blkhdr *d_hdr, float *d_pcm)
{
	if (!pl)
		return ACMHIP_ERR_ARG;
	if (pl->pk_chunks) {
		set_err("acmhip_plan_launch_f32: a packed arena is bound (acmhip_plan_bind_packed); the packed form has no float32 build");
		return ACMHIP_ERR_ARG;
	}
	return plan_launch(pl, d_idx, d_hdr, reinterpret_cast<int16_t *>(d_pcm), ACMK_FMT_F32);
}

extern "C" int acmhip_plan_bind_packed(acmhip_plan *pl, const acmhip_packed_chunk *d_chunks, const uint8_t *d_blob)
{
	if (!pl)
		return ACMHIP_ERR_ARG;
	if ((d_chunks == nullptr) != (d_blob == nullptr)) {
		set_err("acmhip_plan_bind_packed: both tables, or none");
		return ACMHIP_ERR_ARG;
	}
	pl->pk_chunks = d_chunks;
	pl->pk_blob = d_blob;
	return ACMHIP_OK;
}

extern "C" int acmhip_plan_bind_mform(acmhip_plan *pl, const uint8_t *d_mform, const acmhip_mform_pair *d_pairs)
{
	if (!pl)
		return ACMHIP_ERR_ARG;
	if ((d_mform == nullptr) != (d_pairs == nullptr)) {
		set_err("acmhip_plan_bind_mform: the arena and its pair table, or neither");
		return ACMHIP_ERR_ARG;
	}
	pl->mform = d_mform;
	pl->mform_pairs = d_pairs;
	return ACMHIP_OK;
}

extern "C" int acmhip_plan_time(acmhip_plan *pl, const int16_t *d_idx, const acmhip_blkhdr *d_hdr,
				int16_t *d_pcm, unsigned fmt, int reps, float *ms_total)
{
	if (!pl || reps < 1 || !ms_total)
		return ACMHIP_ERR_ARG;
	hipEvent_t a, b;
	HIPTRY(hipEventCreate(&a));
	HIPTRY(hipEventCreate(&b));
	HIPTRY(hipEventRecord(a, pl->dev->stream));
	int rc = ACMHIP_OK;
	for (int i = 0; i < reps && rc == ACMHIP_OK; i++)
		rc = acmhip_plan_launch(pl, d_idx, d_hdr, d_pcm, fmt);
	hipError_t e = hipEventRecord(b, pl->dev->stream);
	if (e == hipSuccess)
		e = hipEventSynchronize(b);
	if (e == hipSuccess)
		e = hipEventElapsedTime(ms_total, a, b);
	(void)hipEventDestroy(a);
	(void)hipEventDestroy(b);
	if (rc != ACMHIP_OK)
		return rc;
	if (e != hipSuccess)
		return hip_fail(e, "event timing");
	return ACMHIP_OK;
}
