/*
 * acm_batch.cpp - batch-of-files front end on one device (include/acm_hip.h).
 *
 * No counterpart in the reference (it decodes one stream at a time on one
 * thread); this is the piece BASELINE.json's north_star adds.
 * Independent streams are bit-parsed by a pool of host threads straight into one
 * pinned staging arena, in arena order.  The arena is cut into chunks of whole
 * streams; as soon as a chunk is parsed it goes H2D, is synthesised by one
 * acmhip_plan_launch and read back on a second HIP stream, while the pool parses
 * the next chunks and then hands finished PCM out to the callers' buffers.  So
 * parsing, H2D, synthesis, D2H and the final copies all overlap.
 */
#include <hip/hip_runtime.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "acm_batch_common.h"
#include "acm_device.h"
#include "acm_hip.h"
#include "acm_stage.h"
#include "libacm.h"

namespace {

using namespace acmbatch;

/* what the run learns about a stream as it is parsed (where it lives: SlotLayout) */
struct Slot {
	acm_stage_info info{};          /* the probed header, then what the parser made of the stream */
	std::vector<acmhip_patch> patches;
	bool ok = false;
	bool host_staged = false;       /* staged by the host reader (its arena slice has to go H2D) */
	/* whole tiles staged in the batch's second form (0: the stream travels as int16): preset from the layout where the device parser
	 * writes the form, else set by the pool; mf_used = bytes of its byte-plane block in use */
	uint32_t pk_ntiles = 0;
	uint64_t mf_used = 0;
	bool mf_fused = false;          /* the form was written by the parsing pass itself (acm_stage_file_mform) */
};

/* a chunk (ChunkLayout) or a block range on its way through the device */
struct Chunk {
	std::atomic<int> unparsed{ 0 };
	std::atomic<uint64_t> pk_used{ 0 };     /* ACM_BATCH_STAGE_PACKED: bytes of this chunk's blob region handed out so far */
	std::atomic<int> back{ 0 };             /* 1 = PCM is in the pinned arena, -1 = the read-back failed */
	acmhip_plan *plan = nullptr;
	hipEvent_t ev[5] = {};                  /* h2d begin, h2d end, kernel end (device stream); d2h begin, d2h end (copy stream) */
};

/* device parsing: the files of one chunk as an upload piece (GroupLayout; copied into the pinned file arena by the pool, sent up as
 * soon as the piece is complete, while the pool copies the next ones).  The walk itself is ONE launch over all streams:
 * a stream's walk is one wavefront's sequential job (~30 ms for two megasamples however many streams walk beside it),
 * and walks launched group by group on streams of their own were measured to slow each other down (last group done
 * after 65 / 86 / 103 ms for 1 / 2 / 4 groups of the 1024-stream level-9 batch: the waves of a later launch land on the
 * compute units - and scalar units - the earlier ones already occupy). */
struct ParseGroup {
	std::atomic<int> uncopied{ 0 };         /* files not yet in the pinned arena */
	hipEvent_t ev[3] = {};                  /* upload begin, upload end; the last piece's third one: parse results on the host */
};

} // namespace

/* what acm_batch_prestage keeps: per item the header, the status, the staged blocks (one allocation for all items, laid out
 * like the batch's own arenas), the H1 patches and the block index (need_blocks + 1 marks per item that is ACM) */
struct acm_batch_prestaged {
	struct Item {
		acm_stage_info info{};
		uint64_t need_blocks = 0, idx_off = 0, hdr_off = 0, marks_off = 0;
		std::vector<acmhip_patch> patches;
		int status = 0;
		bool ok = false;
	};
	std::vector<Item> items;
	std::vector<const uint8_t *> data;      /* the file images the items pointed at, and their lengths (identity check in acm_batch_decode) */
	std::vector<size_t> len;
	int16_t *idx = nullptr;
	acmhip_blkhdr *hdr = nullptr;
	std::vector<acm_block_mark> marks;
	size_t idx_cap = 0, hdr_cap = 0;        /* bytes */
	int force_chans = 0;
};

namespace {
/* Staging buffers of prestaged groups are a hundred megabytes each and live for milliseconds: handing them back to the C
 * library means an munmap (10 ms for 200 MB of touched pages, on the thread that feeds the device) and a fresh set of page
 * faults for the next group.  A few of them are kept here instead and handed out again, best fit. */
struct StageCache {
	struct Buf {
		void *mem;
		size_t cap;
	};
	std::mutex m;
	std::vector<Buf> bufs;
	size_t bytes = 0;
	static constexpr size_t MAX_BUFS = 8, MAX_BYTES = (size_t)1 << 30;

	void *get(size_t want, size_t *cap)
	{
		{
			std::lock_guard<std::mutex> g(m);
			size_t best = bufs.size();
			for (size_t k = 0; k < bufs.size(); k++)
				if (bufs[k].cap >= want && (best == bufs.size() || bufs[k].cap < bufs[best].cap))
					best = k;
			if (best != bufs.size() && bufs[best].cap <= 2 * want + (1u << 20)) {
				const Buf b = bufs[best];
				bufs.erase(bufs.begin() + (long)best);
				bytes -= b.cap;
				*cap = b.cap;
				return b.mem;
			}
		}
		*cap = want;
		return malloc(want);
	}
	void put(void *mem, size_t cap)
	{
		if (!mem)
			return;
		{
			std::lock_guard<std::mutex> g(m);
			if (bufs.size() < MAX_BUFS && bytes + cap <= MAX_BYTES) {
				bufs.push_back(Buf{ mem, cap });
				bytes += cap;
				return;
			}
		}
		free(mem);
	}
};
StageCache g_stage_cache;
}

extern "C" void acm_batch_prestage_free(acm_batch_prestaged *p)
{
	if (!p)
		return;
	if (p->idx && p->idx_cap)
		g_stage_cache.put(p->idx, p->idx_cap);
	if (p->hdr && p->hdr_cap)
		g_stage_cache.put(p->hdr, p->hdr_cap);
	delete p;
}

extern "C" int acm_batch_prestage(const acm_batch_item *items, size_t n, const acm_batch_opts *opts_in, acm_batch_prestaged **out, double *seconds)
{
	if (!out || (n && !items))
		return ACMHIP_ERR_ARG;
	*out = nullptr;
	const auto t0 = clk::now();
	acm_batch_opts opts{};
	if (opts_in)
		opts = *opts_in;
	acm_batch_prestaged *p = new (std::nothrow) acm_batch_prestaged;
	if (!p)
		return ACMHIP_ERR_NOMEM;
	p->items.resize(n);
	p->data.resize(n);
	p->len.resize(n);
	p->force_chans = opts.force_chans;
	const int threads_wanted = opts.threads > 0 ? opts.threads : default_threads();
	Pool pool((int)std::min<size_t>((size_t)threads_wanted, std::max<size_t>(1, n)));
	pool.run(n, [&](size_t i) {
		acm_batch_prestaged::Item &s = p->items[i];
		p->data[i] = items[i].data;
		p->len[i] = items[i].len;
		s.status = acm_stage_probe(items[i].data, items[i].len, opts.force_chans, &s.info);
		s.ok = s.status == ACM_OK;
	});
	Int16Arenas arenas;
	uint64_t marks_total = 0;
	for (size_t i = 0; i < n; i++)
		if (p->items[i].ok) {
			arenas.place(p->items[i].info, items[i].len, &p->items[i].need_blocks, &p->items[i].idx_off, &p->items[i].hdr_off);
			p->items[i].marks_off = marks_total;
			marks_total += p->items[i].need_blocks + 1;
		}
	p->marks.resize(marks_total);
	p->idx = static_cast<int16_t *>(g_stage_cache.get(std::max<uint64_t>(arenas.idx_total, 1) * sizeof(int16_t), &p->idx_cap));
	p->hdr = static_cast<acmhip_blkhdr *>(g_stage_cache.get(std::max<uint64_t>(arenas.hdr_total, 1) * sizeof(acmhip_blkhdr), &p->hdr_cap));
	if (!p->idx || !p->hdr) {
		acm_batch_prestage_free(p);
		return ACMHIP_ERR_NOMEM;
	}
	pool.run(n, [&](size_t i) {
		acm_batch_prestaged::Item &s = p->items[i];
		if (!s.ok)
			return;
		acmstage::Staged st;
		const int r = acmstage::stage_file(items[i].data, items[i].len, opts.force_chans, p->idx + s.idx_off, p->hdr + s.hdr_off, s.need_blocks,
						   p->marks.data() + s.marks_off, nullptr, &st);
		if (r != ACM_OK) {
			s.status = r;
			s.ok = false;
			return;
		}
		s.info = st.info;
		s.patches = std::move(st.patches);
		s.status = st.info.end_status;
	});
	if (seconds)
		*seconds = secs(t0, clk::now());
	*out = p;
	return ACMHIP_OK;
}

extern "C" int acm_batch_prestaged_index(const acm_batch_prestaged *p, size_t i, const acm_block_mark **marks, uint32_t *blocks, int32_t *end_status)
{
	if (!p || i >= p->items.size() || !marks || !blocks || !end_status)
		return ACMHIP_ERR_ARG;
	const acm_batch_prestaged::Item &s = p->items[i];
	*marks = s.ok ? p->marks.data() + s.marks_off : nullptr;
	*blocks = s.ok ? s.info.blocks : 0;
	*end_status = s.ok ? s.info.end_status : 0;
	return s.ok ? ACM_OK : s.status;
}

extern "C" uint64_t acm_batch_pcm_words(const acm_batch_item *items, size_t n, int force_chans)
{
	Int16Arenas arenas;
	for (size_t i = 0; items && i < n; i++) {
		acm_stage_info info;
		uint64_t blocks, idx_off, hdr_off;
		if (acm_stage_probe(items[i].data, items[i].len, force_chans, &info) == ACM_OK)
			arenas.place(info, items[i].len, &blocks, &idx_off, &hdr_off);
	}
	return arenas.idx_total;
}

namespace {

constexpr size_t STRIPE_BATCH = 32;             /* files per stripe copy task */
constexpr size_t STRIPE_MARGIN = 2;             /* range r is walked behind stripe r + STRIPE_MARGIN (BatchRun::upload_and_walk) */
struct Span { uint64_t at, len; };

/* ACM_BATCH_TRACE: host-side timeline on stderr */
bool tracing()
{
	static const bool trace = getenv("ACM_BATCH_TRACE") != nullptr;
	return trace;
}

#define BNOTE(...) do { if (trace) { fprintf(stderr, "[batch %8.3f ms] ", secs(t0, clk::now()) * 1e3); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

/* One acm_batch_decode / acm_batch_decode_indexed call behind the arena lock: the device-side state of the pipeline over a BatchLayout it only reads.  The stages
 * are called once each, in the order of acm_batch_decode; a stage that fails returns its code and the destructor does the rest. */
class BatchRun {
public:
	BatchRun(acmhip_device *dev_, acm_batch_item *items_, size_t n_, const acm_batch_opts &opts_, const BatchLayout &L_, Pool &pool_,
		 const std::vector<LayoutItem> &probed, acm_batch_index_out *index_, clk::time_point t0_, clk::time_point t_hdr_)
		: lock(dev_), dev(dev_), items(items_), n(n_), index(index_), opts(opts_), pre(opts_.prestaged), L(L_), pool(pool_), t0(t0_), t_hdr(t_hdr_),
		  out_f32((opts_.flags & ACM_BATCH_PCM_F32) != 0), R(L_.R), nd(L_.dev_ids.size()), nbat((nd + STRIPE_BATCH - 1) / STRIPE_BATCH),
		  st_main((hipStream_t)acmhip_device_stream(dev_)), slots(n_), chunks(L_.chunks.size()), rchunks(R > 1 ? R : 0),
		  groups(L_.groups.size()), ev_stripe(R > 1 ? R + 1 : 0, nullptr), stripe_uncopied(R > 1 ? new std::atomic<int>[R] : nullptr),
		  planned(L_.chunks.size(), 0), replan(L_.chunks.size(), 0)
	{
		for (size_t i = 0; i < n; i++) {
			slots[i].info = probed[i].info;
			slots[i].ok = probed[i].ok;
			slots[i].pk_ntiles = L.slots[i].pk_ntiles;
		}
	}
	/* what every early return needs: the pool stopped, the streams idle, events and plans gone, the arenas unlocked (ArenaLock, last) */
	~BatchRun()
	{
		if (pool_busy) {
			{
				std::lock_guard<std::mutex> g(m);
				aborted = true;
			}
			cv.notify_all();
			pool.wait();
		}
		if (st_up)
			(void)hipStreamSynchronize(st_up);
		if (st_parse)
			(void)hipStreamSynchronize(st_parse);
		(void)hipStreamSynchronize(st_main);
		if (st_copy)
			(void)hipStreamSynchronize(st_copy);
		for (ParseGroup &g : groups)
			drop_unit(nullptr, g.ev, 3);
		drop_unit(nullptr, ev_stripe.data(), ev_stripe.size());
		for (std::vector<Chunk> *v : { &chunks, &rchunks })
			for (Chunk &ch : *v)
				drop_unit(ch.plan, ch.ev, 5);
	}
	int acquire();
	int start_pool();
	int plan_device_chunks();
	int upload_and_walk();
	int feed_chunks();
	int finish();
	void roll_up(acm_batch_timing *timing);

private:
	void host_pack(size_t i);
	void host_mform(size_t i);
	void host_stage_int16(size_t i);
	void index_staged(size_t i, int rc, const acm_stage_info &info)    /* the host reader went over stream i with index[i].marks in hand */
	{
		if (!index)
			return;
		index[i].status = rc;
		index[i].blocks = rc == ACM_OK ? info.blocks : 0;
		index[i].end_status = rc == ACM_OK ? info.end_status : 0;
	}
	void host_stage(size_t i)
	{
		host_stage_int16(i);
		host_pack(i);
		host_mform(i);
	}
	void copy_stripe_task(size_t task);
	void copy_file_task(size_t k);
	void host_parse_task(size_t task);
	void copy_out_task(size_t task);
	int build_plan(size_t c);
	int cut_range_plan(size_t r);
	int launch_range(size_t r, size_t stripes_up);
	int settle();
	hipError_t upload_spans(uint8_t *d_base, const uint8_t *h_base);
	int upload_forms_and_tails(size_t c);
	int upload_int16_slice(size_t c);
	int upload_host_staged(size_t c);
	int fix_up();
	int launch(acmhip_plan *plan) { return launch_plan(plan, out_f32, d_idx, d_hdr, d_pcm, opts.fmt); }
	bool second_form() const { return L.stage_mform || L.dev_mform; }       /* the batch's second form is the byte-plane one */
	void announce(size_t unit)                      /* the read-back of chunk / range `unit` is queued: the copy-out may wait for it */
	{
		{
			std::lock_guard<std::mutex> g(m);
			issued.store(unit + 1, std::memory_order_release);
		}
		cv.notify_all();
	}

	ArenaLock lock;
	acmhip_device *const dev;
	acm_batch_item *const items;
	const size_t n;
	acm_batch_index_out *const index;       /* null: nobody asked for the block index */
	const acm_batch_opts &opts;
	const acm_batch_prestaged *const pre;
	const BatchLayout &L;
	Pool &pool;
	acm_batch_timing tm{};
	const bool trace = tracing();
	const clk::time_point t0, t_hdr;
	clk::time_point t_alloc, t_parsed, t_dev_parsed;
	const bool out_f32;
	const size_t R, nd, nbat;
	int16_t *h_idx = nullptr, *h_pcm = nullptr, *d_idx = nullptr, *d_pcm = nullptr;
	uint32_t *d_colpos = nullptr, *d_blkoff = nullptr;
	acmhip_blkhdr *h_hdr = nullptr, *d_hdr = nullptr;
	acm_block_mark *h_marks = nullptr, *d_marks = nullptr;  /* the index as a by-product of the device walk: parallel to the header arena */
	uint8_t *h_files = nullptr, *d_files = nullptr, *h_jobs = nullptr, *d_jobs = nullptr, *d_stage = nullptr;
	uint8_t *h_pkblob = nullptr, *d_pkblob = nullptr;
	acmhip_packed_chunk *h_pkchunk = nullptr, *d_pkchunk = nullptr;
	const AcmParseResult *results = nullptr;        /* the device parser's verdicts in the pinned job arena, their flags behind them */
	const uint32_t *flags = nullptr;
	hipStream_t st_main, st_copy = nullptr;
	hipStream_t st_up = nullptr, st_parse = nullptr;        /* file uploads piece by piece; the walk + column kernels */
	std::mutex m;
	std::condition_variable cv;
	std::atomic<size_t> issued{ 0 };                /* chunks whose read-back has been queued */
	std::atomic<size_t> parsed{ 0 };
	bool aborted = false, pool_busy = false, settled = false;
	std::vector<Slot> slots;
	std::vector<Chunk> chunks, rchunks;             /* block ranges: plan, events and read-back state of each */
	std::vector<ParseGroup> groups;
	std::vector<hipEvent_t> ev_stripe;              /* [0] = first stripe's upload begins, [s + 1] = stripe s is in place */
	std::unique_ptr<std::atomic<int>[]> stripe_uncopied;
	std::vector<char> planned, replan;
	std::vector<size_t> redo;               /* block ranges: streams the device flagged - decoded again from the host reader's staging */
	std::vector<Span> spans;
	uint64_t max_columns = 0;
	hipEvent_t ev_parsed = nullptr;
	size_t ncopy = 0, nparse = 0;
};

/* Arenas (they live in the device handle and are reused by the next batch), streams and events.  Needs nothing but the layout */
int BatchRun::acquire()
{
	const uint64_t idx_total = L.idx_total, hdr_total = L.hdr_total;
	ACM_TRY(acmhip_copy_stream(dev, (void **)&st_copy));
	if (!L.dev_parse)                       /* with device parsing the host staging arenas come later, and only if a stream needs them */
		ACM_TRY(host_arenas(dev, idx_total, hdr_total, &h_idx, &h_hdr));
	if (L.stage_packed) {
		const uint64_t pk_blob_bytes = idx_total * sizeof(int16_t) + 4096;     /* region of chunk c = bytes [2 idx_begin, 2 idx_end) */
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_PKBLOB, pk_blob_bytes, (void **)&h_pkblob));
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_PKBLOB, pk_blob_bytes, (void **)&d_pkblob));
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_PKCHUNK, L.pk_chunks_total * sizeof(acmhip_packed_chunk), (void **)&h_pkchunk));
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_PKCHUNK, L.pk_chunks_total * sizeof(acmhip_packed_chunk), (void **)&d_pkchunk));
	}
	if (L.stage_mform) {
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_PKBLOB, L.mf_total, (void **)&h_pkblob));
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_PKBLOB, L.mf_total, (void **)&d_pkblob));
		/* (+ 32 entries: the kernel's scalar loads fetch whole groups) */
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_PKCHUNK, (L.mf_pairs_total + 32) * sizeof(acmhip_mform_pair), (void **)&h_pkchunk));
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_PKCHUNK, (L.mf_pairs_total + 32) * sizeof(acmhip_mform_pair), (void **)&d_pkchunk));
	}
	if (L.dev_mform) {
		/* (+ 128 KB: a stream whose walk stops early has its unwritten pair-table entries parked right behind its last staged block,
		 * acm_parse.hip, and a chunk read from there may reach two pairs on - behind the last stream that is behind the arena's contents) */
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_PKBLOB, L.mf_total + (128u << 10), (void **)&d_pkblob));
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_PKCHUNK, (L.mf_pairs_total + 32) * sizeof(acmhip_mform_pair), (void **)&d_pkchunk));
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_BLKOFF, hdr_total * sizeof(uint32_t), (void **)&d_blkoff));
	}
	if (!L.keep_on_device && !L.direct_out)
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_PCM, L.pcm_arena_words * sizeof(int16_t), (void **)&h_pcm));
	ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_IDX, idx_total * sizeof(int16_t), (void **)&d_idx));
	ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_HDR, hdr_total * sizeof(acmhip_blkhdr), (void **)&d_hdr));
	if (L.keep_on_device)
		d_pcm = static_cast<int16_t *>(opts.d_pcm);
	else
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_PCM, L.pcm_arena_words * sizeof(int16_t), (void **)&d_pcm));
	if (nd) {
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_FILES, L.files_total, (void **)&h_files));
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_FILES, L.files_total, (void **)&d_files));
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_COLPOS, L.cols_total * sizeof(uint32_t), (void **)&d_colpos));
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_JOBS, L.stripe_tab_off + L.stripe_tab_bytes, (void **)&h_jobs));
		ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_JOBS, L.stripe_tab_off + L.stripe_tab_bytes, (void **)&d_jobs));
		if (R > 1)
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_STAGE, L.files_total, (void **)&d_stage));
		if (index) {
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_D_MARKS, hdr_total * sizeof(acm_block_mark), (void **)&d_marks));
			ACM_TRY(acmhip_arena_get(dev, ACM_ARENA_H_MARKS, hdr_total * sizeof(acm_block_mark), (void **)&h_marks));
		}
	}
	for (std::vector<Chunk> *v : { &chunks, &rchunks })
		for (Chunk &ch : *v)
			ACM_TRY(make_events(ch.ev, 5));
	if (!groups.empty()) {
		ACM_TRY(acmhip_aux_stream(dev, ACM_AUX_STREAMS - 1, (void **)&st_up));
		/* block ranges: walk r, its columns and its synthesis (0.2 ms) follow each other anyway - one stream; what must never
		 * share a hardware queue is the upload, the read-back and the kernels (the runtime maps streams onto a handful of
		 * queues: an upload queued behind a 5 ms read-back on the same one arrives 5 ms late, every stripe of it) */
		if (R > 1)
			st_parse = st_main;
		else
			ACM_TRY(acmhip_aux_stream(dev, 0, (void **)&st_parse));
	}
	for (ParseGroup &g : groups)
		ACM_TRY(make_events(g.ev, 3));
	ACM_TRY(make_events(ev_stripe.data(), ev_stripe.size()));
	t_alloc = t_parsed = t_dev_parsed = clk::now();
	tm.alloc_s = secs(t_hdr, t_alloc);
	BNOTE("headers %.3f ms, arenas + events %.3f ms; %zu chunks, %zu parse groups", secs(t0, t_hdr) * 1e3, tm.alloc_s * 1e3, chunks.size(), groups.size());
	return ACMHIP_OK;
}

/* the packed half of the host stager: the whole tiles of a clean stream, from the int16 rows the reader has just written
 * (they are still in the cache), into the chunk's region of the blob arena.  Needs host_stage_int16(i) done */
void BatchRun::host_pack(size_t i)
{
	Slot &s = slots[i];
	const SlotLayout &p = L.slots[i];
	if (!L.stage_packed || !s.ok || !p.pk_chunk_cap || !s.patches.empty() || items[i].words == 0)
		return;
	const int tr = acmhip_packed_tile_rows(s.info.level);
	const uint64_t full_rows = std::min<uint64_t>((uint64_t)s.info.blocks * s.info.rows, items[i].words >> s.info.level);
	const uint64_t ntiles = full_rows / (uint64_t)tr, slots_per = (uint64_t)acmhip_packed_slots(s.info.level);
	if (ntiles == 0 || ntiles * slots_per > p.pk_chunk_cap)
		return;
	uint64_t bound = 0;
	if (acmhip_pack_bound(s.info.level, ntiles, &bound) != ACMHIP_OK)
		return;
	static thread_local std::vector<uint8_t> scratch;
	if (scratch.size() < bound)
		scratch.resize(bound);
	uint64_t bytes = 0;
	acmhip_packed_chunk *tc = h_pkchunk + p.pk_chunk_off;
	if (acmhip_pack_tiles(s.info.level, h_idx + p.idx_off, ntiles, tc, scratch.data(), 0, &bytes) != ACMHIP_OK)
		return;
	const ChunkLayout &cl = L.chunks[p.chunk];
	const uint64_t region = cl.idx_begin * sizeof(int16_t), region_len = (cl.idx_end - cl.idx_begin) * sizeof(int16_t);
	const uint64_t at = chunks[p.chunk].pk_used.fetch_add((bytes + 15) & ~15ull);
	if (at + bytes > region_len)
		return;                 /* does not fit beside the others: this stream travels as int16 (its entries stay unused) */
	memcpy(h_pkblob + region + at, scratch.data(), bytes);
	for (uint64_t k = 0; k < ntiles * slots_per; k++)
		if (tc[k].kind)
			tc[k].blob_off16 += (uint32_t)((region + at) / 16);
	s.pk_ntiles = (uint32_t)ntiles;
}

/* the byte-plane half: the whole tiles of a clean stream, re-ordered from the int16 rows the reader has just written.  Needs
 * host_stage_int16(i) done; does nothing where that pass wrote the form itself */
void BatchRun::host_mform(size_t i)
{
	Slot &s = slots[i];
	const SlotLayout &p = L.slots[i];
	if (!L.stage_mform || !s.ok || !p.mf_rows_cap || !s.patches.empty() || items[i].words == 0 || s.mf_fused)
		return;
	const int tr = acmhip_mform_tile_rows(s.info.level);
	const uint64_t full_rows = std::min<uint64_t>((uint64_t)s.info.blocks * s.info.rows, items[i].words >> s.info.level);
	uint64_t ntiles = full_rows / (uint64_t)tr;
	if ((ntiles * (uint64_t)tr) & 1)
		ntiles--;                       /* the form is written pair by pair (tiles of one row: an even number of them) */
	if (ntiles == 0 || ntiles * (uint64_t)tr > p.mf_rows_cap)
		return;
	if (acmhip_mform_rows(s.info.level, h_idx + p.idx_off, ntiles * (uint64_t)tr, h_pkblob + p.mf_off, p.mf_off,
			      reinterpret_cast<acmhip_mform_pair *>(h_pkchunk) + p.mf_pair_off, &s.mf_used) != ACMHIP_OK)
		return;
	s.pk_ntiles = (uint32_t)ntiles;
}

/* the exact host reader, one stream.  Needs the host staging arenas (host_arenas) and, with a second form, its arenas */
void BatchRun::host_stage_int16(size_t i)
{
	Slot &s = slots[i];
	const SlotLayout &p = L.slots[i];
	acm_batch_item &it = items[i];
	acm_stage_info info{};
	acm_block_mark *const marks = index ? index[i].marks : nullptr;        /* filled where the reader begins a block */
	if (pre) {
		/* parsed already: the staged blocks - and their marks - only have to move into the upload arenas */
		const acm_batch_prestaged::Item &ps = pre->items[i];
		if (!ps.ok) {
			it.status = ps.status;
			s.ok = false;
			index_staged(i, ps.status, info);
			return;
		}
		const uint64_t bl = (uint64_t)ps.info.rows * ps.info.cols;
		if (ps.need_blocks != p.need_blocks || ps.info.blocks > p.need_blocks) {      /* cannot happen for the same bytes */
			it.status = ACM_ERR_OTHER;
			s.ok = false;
			index_staged(i, ACM_ERR_OTHER, info);
			return;
		}
		if (marks)
			memcpy(marks, pre->marks.data() + ps.marks_off, ((size_t)ps.info.blocks + 1) * sizeof(acm_block_mark));
		index_staged(i, ACM_OK, ps.info);
		memcpy(h_idx + p.idx_off, pre->idx + ps.idx_off, ps.info.blocks * bl * sizeof(int16_t));
		memcpy(h_hdr + p.hdr_off, pre->hdr + ps.hdr_off, ps.info.blocks * sizeof(acmhip_blkhdr));
		s.patches = ps.patches;
		s.info = ps.info;
		s.host_staged = true;
		it.status = ps.info.end_status;
		it.words = deliverable_words(ps.info.total_values, bl, ps.info.channels, ps.info.blocks);
		return;
	}
	/* one pass, patches (normally none) included.  With ACM_BATCH_STAGE_BYTEPLANE it also writes the byte-plane form, block by block
	 * out of the cache (acm_stage_file_mform), where the stream can have it */
	const bool fuse = L.stage_mform && p.mf_rows_cap;
	const acmstage::MformArena mf{ fuse ? h_pkblob + p.mf_off : nullptr, p.mf_off,
				       fuse ? reinterpret_cast<acmhip_mform_pair *>(h_pkchunk) + p.mf_pair_off : nullptr };
	acmstage::Staged st;
	const int r = acmstage::stage_file(it.data, it.len, opts.force_chans, h_idx + p.idx_off, h_hdr + p.hdr_off, p.need_blocks, marks,
					   fuse ? &mf : nullptr, &st);
	if (r == ACM_OK && st.mf_rows && st.mf_rows <= p.mf_rows_cap) {
		s.pk_ntiles = (uint32_t)(st.mf_rows / (uint64_t)acmhip_mform_tile_rows(st.info.level));
		s.mf_used = st.mf_bytes;
		s.mf_fused = true;
	}
	info = st.info;
	s.patches = std::move(st.patches);
	index_staged(i, r, info);
	if (r != ACM_OK) {
		it.status = r;
		s.ok = false;
		return;
	}
	s.info = info;
	s.host_staged = true;
	it.status = info.end_status;
	it.words = deliverable_words(info.total_values, (uint64_t)info.rows * info.cols, info.channels, info.blocks);
}

/* 2a / 2b. The device parser's tables into the pinned job arena; then the pool: files of the device-parsed streams into the pinned arena
 * (group order, or stripe by stripe), host parsing in arena order, then finished PCM out to the callers' buffers as the chunks come back.
 * Whatever the device flags later is re-parsed by the exact host reader on the feeding thread (rare).  Needs acquire() */
int BatchRun::start_pool()
{
	if (nd) {
		memcpy(h_jobs, L.jobs.data(), nd * sizeof(AcmParseJob));
		results = reinterpret_cast<const AcmParseResult *>(h_jobs + L.jobs_bytes);
		flags = reinterpret_cast<const uint32_t *>(results + nd);
		for (size_t g = 0; g < groups.size(); g++)
			groups[g].uncopied.store((int)(L.groups[g].k_last - L.groups[g].k_first));
	}
	if (R > 1) {
		memcpy(h_jobs + L.stripe_tab_off, L.stripe_at.data(), L.stripe_tab_bytes);
		for (size_t s = 0; s < R; s++)
			stripe_uncopied[s].store((int)nbat);
	}
	if (L.dev_parse && !L.host_ids.empty()) {
		const auto ta = clk::now();
		ACM_TRY(host_arenas(dev, L.idx_total, L.hdr_total, &h_idx, &h_hdr));
		tm.alloc_s += secs(ta, clk::now());
	}
	tm.host_parsed = L.host_ids.size();
	for (size_t i : L.host_ids)
		chunks[L.slots[i].chunk].unparsed.fetch_add(1);
	t_parsed = clk::now();
	ncopy = groups.empty() ? 0 : R > 1 ? R * nbat : nd;
	nparse = L.host_ids.size();
	pool_busy = true;
	pool.start(ncopy + nparse + L.out_ids.size() * R, [this](size_t task) {
		if (task < ncopy && R > 1)
			copy_stripe_task(task);
		else if (task < ncopy)
			copy_file_task(task);
		else if (task - ncopy < nparse)
			host_parse_task(task - ncopy);
		else
			copy_out_task(task - ncopy - nparse);
	});
	return ACMHIP_OK;
}

/* pool, block ranges: one stripe of STRIPE_BATCH files into the pinned file arena - stripe-major, stripe 0 of every file first */
void BatchRun::copy_stripe_task(size_t task)
{
	const size_t s = task / nbat, k0 = task % nbat * STRIPE_BATCH;
	for (size_t k = k0; k < std::min(nd, k0 + STRIPE_BATCH); k++) {
		const acm_batch_item &it = items[L.dev_ids[k]];
		const uint64_t lo = acmk_stripe_bound((uint32_t)it.len, (uint32_t)s, (uint32_t)R),
			       hi = acmk_stripe_bound((uint32_t)it.len, (uint32_t)s + 1, (uint32_t)R);
		const uint64_t have = it.len > lo ? std::min<uint64_t>(it.len, hi) - lo : 0;       /* file bytes in this stripe; then the slot's zero tail */
		copy_zero_tail(h_files + L.stripe_at[s * nd + k], it.data + lo, have, hi - lo);
	}
	if (stripe_uncopied[s].fetch_sub(1) == 1) {
		std::lock_guard<std::mutex> g(m);
		cv.notify_all();
	}
}

/* pool: the file of device-parsed stream dev_ids[k] into its slot of the pinned file arena */
void BatchRun::copy_file_task(size_t k)
{
	const size_t i = L.dev_ids[k];
	copy_zero_tail(h_files + L.slots[i].file_off, items[i].data, items[i].len, file_slot_bytes(items[i].len));
	if (groups[L.slots[i].chunk].uncopied.fetch_sub(1) == 1) {
		std::lock_guard<std::mutex> g(m);
		cv.notify_all();
	}
}

/* pool: the host reader over stream host_ids[task] */
void BatchRun::host_parse_task(size_t task)
{
	const size_t i = L.host_ids[task];
	host_stage(i);
	if (parsed.fetch_add(1) + 1 == nparse)
		t_parsed = clk::now();
	if (chunks[L.slots[i].chunk].unparsed.fetch_sub(1) == 1) {
		std::lock_guard<std::mutex> g(m);
		cv.notify_all();
	}
}

/* pool, copy-out: a whole stream of its chunk - or, with block ranges, one range's piece of a stream - once the read-back of that
 * chunk / range has been queued (announce) and has ended */
void BatchRun::copy_out_task(size_t task)
{
	const size_t piece = task / L.out_ids.size();           /* 0 without ranges */
	const size_t i = L.out_ids[task % L.out_ids.size()];
	const Slot &s = slots[i];
	const SlotLayout &p = L.slots[i];
	const size_t unit = R > 1 ? piece : p.chunk;
	Chunk &ch = R > 1 ? rchunks[piece] : chunks[p.chunk];
	if (ch.back.load(std::memory_order_acquire) == 0) {     /* first one here waits for the chunk */
		if (issued.load(std::memory_order_acquire) <= unit) {
			std::unique_lock<std::mutex> g(m);
			cv.wait(g, [&]() { return aborted || issued.load() > unit; });
			if (aborted)
				return;
		}
		const bool good = hipEventSynchronize(ch.ev[4]) == hipSuccess;
		ch.back.store(good ? 1 : -1, std::memory_order_release);
		BNOTE("%s %zu is back", R > 1 ? "range" : "chunk", unit);
	}
	if (ch.back.load(std::memory_order_acquire) < 0 || !s.ok)
		return;
	if (R > 1) {
		/* the piece starts where the stream's earlier ranges end (they are whole blocks); a stream the device flags
		 * later is decoded again from the host reader's staging and copied out whole (fix-up, below) */
		const uint64_t bl = (uint64_t)s.info.rows * s.info.cols;
		const uint64_t lo = (uint64_t)acmk_range_bound((uint32_t)p.need_blocks, (uint32_t)piece, (uint32_t)R, p.range_unit) * bl, len = L.piece_len[piece * n + i];
		if (lo >= items[i].pcm_cap || len == 0)
			return;
		memcpy(items[i].pcm + lo, h_pcm + L.piece_off[piece * n + i], std::min<uint64_t>(len, items[i].pcm_cap - lo) * sizeof(int16_t));
		return;
	}
	if (items[i].words == 0)
		return;
	const uint64_t w = std::min<uint64_t>(items[i].words, items[i].pcm_cap);
	memcpy(items[i].pcm, h_pcm + p.pcm_off, w * sizeof(int16_t));
}

/* the launch plan of chunk c from what is known about its streams right now: every stream of the chunk is parsed (or, ahead of the
 * device parser, assumed clean: plan_device_chunks) */
int BatchRun::build_plan(size_t c)
{
	Chunk &ch = chunks[c];
	PlanStreams ps;
	std::vector<acmhip_packed_stream> packed;
	for (size_t i = L.chunks[c].first; i < L.chunks[c].last; i++) {
		const Slot &s = slots[i];
		const SlotLayout &p = L.slots[i];
		if (!s.ok || items[i].words == 0)
			continue;
		if (second_form())
			packed.push_back(acmhip_packed_stream{ p.mf_pair_off, s.pk_ntiles, ACMHIP_FORM_BYTEPLANE });
		else
			packed.push_back(acmhip_packed_stream{ p.pk_chunk_off, s.pk_ntiles, ACMHIP_FORM_PACKED });
		ps.add(s.info, p.idx_off, p.hdr_off, p.pcm_off, s.info.blocks * s.info.rows, 0, items[i].words, s.patches);
	}
	if (ch.plan) {
		acmhip_plan_destroy(ch.plan);
		ch.plan = nullptr;
	}
	if (ps.descs.empty())
		return ACMHIP_OK;
	if (!L.stage_packed && !second_form())
		return acmhip_plan_create(dev, ps.descs.data(), ps.descs.size(), ps.patches.data(), ps.patches.size(), opts.plan_flags, &ch.plan);
	/* (a chunk's byte-plane streams are never launched without their form: no records over int16 rows they may not have) */
	ACM_TRY(acmhip_plan_create_packed(dev, ps.descs.data(), ps.descs.size(), packed.data(), ps.patches.data(), ps.patches.size(),
					  opts.plan_flags | (second_form() ? ACMHIP_PLAN_FORM_ONLY : 0u), &ch.plan));
	return second_form() ? acmhip_plan_bind_mform(ch.plan, d_pkblob, reinterpret_cast<const acmhip_mform_pair *>(d_pkchunk))
			     : acmhip_plan_bind_packed(ch.plan, d_pkchunk, d_pkblob);
}

/* block ranges: one plan per range over every stream's piece (a window of the stream that starts at the range's first row;
 * the staged rows in front of it are on the device by then: earlier ranges).  Cut right behind the launch of the range's walk,
 * which takes the device longer than the tables take the host; their upload is only queued (ACMHIP_PLAN_UPLOAD_ASYNC), so a
 * table copy that shares a hardware queue with a walk kernel holds up nothing but the synthesis that waits for that walk anyway */
int BatchRun::cut_range_plan(size_t r)
{
	PlanStreams ps;
	std::vector<acmhip_packed_stream> packed;
	for (size_t i = 0; i < n; i++) {
		const Slot &s = slots[i];
		const SlotLayout &p = L.slots[i];
		if (!s.ok || L.piece_len[r * n + i] == 0)
			continue;
		packed.push_back(acmhip_packed_stream{ p.mf_pair_off, s.pk_ntiles, ACMHIP_FORM_BYTEPLANE });
		ps.add(s.info, p.idx_off, p.hdr_off, L.piece_off[r * n + i],
		       acmk_range_bound((uint32_t)p.need_blocks, (uint32_t)r + 1u, (uint32_t)R, p.range_unit) * s.info.rows,
		       acmk_range_bound((uint32_t)p.need_blocks, (uint32_t)r, (uint32_t)R, p.range_unit) * s.info.rows, L.piece_len[r * n + i], {});
	}
	if (ps.descs.empty())
		return ACMHIP_OK;
	const unsigned pf = opts.plan_flags | ACMHIP_PLAN_UPLOAD_ASYNC;
	if (!L.dev_mform)
		return acmhip_plan_create(dev, ps.descs.data(), ps.descs.size(), nullptr, 0, pf, &rchunks[r].plan);
	/* every range is a plan of windows; a window of a stream the device stages in the byte-plane form goes to the lean kernels */
	ACM_TRY(acmhip_plan_create_packed(dev, ps.descs.data(), ps.descs.size(), packed.data(), nullptr, 0, pf | ACMHIP_PLAN_FORM_ONLY, &rchunks[r].plan));
	return acmhip_plan_bind_mform(rchunks[r].plan, d_pkblob, reinterpret_cast<const acmhip_mform_pair *>(d_pkchunk));
}

/* chunks made of device-parsed streams only: their plans are cut NOW, from what the headers promise (a stream the
 * device parser flags later gets its chunk's plan rebuilt), while the queues are still empty - a plan's small table
 * uploads otherwise wait behind whatever long walk kernel shares their hardware queue.  Needs acquire(); nothing of these chunks is
 * parsed yet */
int BatchRun::plan_device_chunks()
{
	if (groups.empty() || R > 1)
		return ACMHIP_OK;
	for (size_t c = 0; c < chunks.size(); c++) {
		const ChunkLayout &cl = L.chunks[c];
		bool all_dev = true;
		for (size_t i = cl.first; i < cl.last; i++)
			all_dev = all_dev && (!slots[i].ok || L.slots[i].on_dev);
		if (!all_dev)
			continue;
		for (size_t i = cl.first; i < cl.last; i++) {
			Slot &s = slots[i];
			if (!s.ok)
				continue;
			s.info.blocks = (uint32_t)L.slots[i].need_blocks;
			items[i].words = deliverable_words(s.info.total_values, (uint64_t)s.info.rows * s.info.cols, s.info.channels, L.slots[i].need_blocks);
		}
		ACM_TRY(build_plan(c));
		planned[c] = 1;
	}
	BNOTE("plans of the all-device chunks built");
	return ACMHIP_OK;
}

/* one block range: the walk + column kernels, and with R > 1 the synthesis and the read-back of what they staged.  Needs the job table on
 * the device and st_parse waiting for the file bytes the range reads (stripes_up of them; 0 = whole files) */
int BatchRun::launch_range(size_t r, size_t stripes_up)
{
	AcmParseResult *d_res = reinterpret_cast<AcmParseResult *>(d_jobs + L.jobs_bytes);
	const acmhip_launch_caps caps = acmhip_device_launch_caps(dev);
	const int e = acmk_launch_parse_range_mf(reinterpret_cast<const AcmParseJob *>(d_jobs), (uint32_t)nd, d_files, d_colpos, d_idx,
						 d_hdr, d_res, reinterpret_cast<uint32_t *>(d_res + nd), max_columns, (uint32_t)r, (uint32_t)R, (uint32_t)stripes_up,
						 L.dev_mform ? d_pkblob : nullptr, L.dev_mform ? reinterpret_cast<uint32_t *>(d_pkchunk) : nullptr,
						 L.dev_mform ? d_blkoff : nullptr, d_marks, caps.parse_slice, caps.parse_grid_x, st_parse);
	if (e != 0)
		return acmhip_report_hip(e, "acmk_launch_parse_range");
	BNOTE("range %zu: walk queued", r);
	if (R == 1)
		return ACMHIP_OK;
	/* range r is staged: synthesise it and read it back while the walk goes on */
	Chunk &rg = rchunks[r];
	ACM_TRY(cut_range_plan(r));
	BNOTE("range %zu: plan cut", r);
	ACM_HIP_TRY(hipEventRecord(rg.ev[1], st_parse));
	ACM_HIP_TRY(hipStreamWaitEvent(st_main, rg.ev[1], 0));
	ACM_HIP_TRY(hipEventRecord(rg.ev[0], st_main));
	if (rg.plan)
		ACM_TRY(launch(rg.plan));
	BNOTE("range %zu: synthesis queued", r);
	ACM_HIP_TRY(hipEventRecord(rg.ev[2], st_main));
	ACM_HIP_TRY(hipStreamWaitEvent(st_copy, rg.ev[2], 0));
	ACM_HIP_TRY(hipEventRecord(rg.ev[3], st_copy));
	if (L.rbase[r + 1] > L.rbase[r])
		ACM_HIP_TRY(hipMemcpyAsync(h_pcm + L.rbase[r], d_pcm + L.rbase[r], (L.rbase[r + 1] - L.rbase[r]) * sizeof(int16_t), hipMemcpyDeviceToHost, st_copy));
	ACM_HIP_TRY(hipEventRecord(rg.ev[4], st_copy));
	BNOTE("range %zu: walk, synthesis and read-back queued", r);
	announce(r);
	return ACMHIP_OK;
}

/* 2c. every piece goes up as soon as its files are in the pinned arena; behind the last one, one walk over all streams - or, with block
 * ranges, stripe by stripe with the ranges' walks, syntheses and read-backs behind them.  Needs start_pool() */
int BatchRun::upload_and_walk()
{
	for (size_t gi = 0; gi < groups.size(); gi++) {
		const GroupLayout &gl = L.groups[gi];
		ParseGroup &g = groups[gi];
		if (gl.k_first == gl.k_last)
			continue;
		max_columns = std::max(max_columns, gl.max_columns);
		ev_parsed = g.ev[2];
		if (R > 1)
			continue;               /* striped upload below */
		{
			std::unique_lock<std::mutex> lk(m);
			cv.wait(lk, [&]() { return g.uncopied.load() == 0; });
		}
		const size_t nj = gl.k_last - gl.k_first;
		ACM_HIP_TRY(hipEventRecord(g.ev[0], st_up));
		ACM_HIP_TRY(hipMemcpyAsync(d_files + gl.file_begin, h_files + gl.file_begin, gl.file_end - gl.file_begin, hipMemcpyHostToDevice, st_up));
		ACM_HIP_TRY(hipMemcpyAsync(d_jobs + gl.k_first * sizeof(AcmParseJob), h_jobs + gl.k_first * sizeof(AcmParseJob), nj * sizeof(AcmParseJob),
					   hipMemcpyHostToDevice, st_up));
		ACM_HIP_TRY(hipEventRecord(g.ev[1], st_up));
		if (gi + 1 == groups.size() || L.groups[gi + 1].k_first == L.groups[gi + 1].k_last)
			BNOTE("files up to piece %zu queued for upload", gi);
	}
	if (!ev_parsed)
		return ACMHIP_OK;
	ACM_HIP_TRY(hipMemsetAsync(d_jobs + L.jobs_bytes + nd * sizeof(AcmParseResult), 0, nd * sizeof(uint32_t), st_parse));   /* the flags */
	if (R == 1) {
		ACM_HIP_TRY(hipEventRecord(ev_parsed, st_up));          /* re-recorded below: here it only orders the walk behind the last upload */
		ACM_HIP_TRY(hipStreamWaitEvent(st_parse, ev_parsed, 0));
		ACM_TRY(launch_range(0, 0));
	} else {
		/* striped upload: stripe s of every file as one transfer + a scatter kernel; the walk of range r may start once
		 * stripe r + STRIPE_MARGIN is in place (a range of blocks ends near the end of its stripe of the bits; a stream whose bit
		 * rate is so uneven that it needs more than the margin is stopped there and taken by the host reader) */
		ACM_HIP_TRY(hipMemcpyAsync(d_jobs, h_jobs, L.jobs_bytes, hipMemcpyHostToDevice, st_up));
		ACM_HIP_TRY(hipMemcpyAsync(d_jobs + L.stripe_tab_off, h_jobs + L.stripe_tab_off, L.stripe_tab_bytes, hipMemcpyHostToDevice, st_up));
		ACM_HIP_TRY(hipEventRecord(ev_stripe[0], st_up));
		for (size_t sp = 0; sp < R; sp++) {
			{
				std::unique_lock<std::mutex> lk(m);
				cv.wait(lk, [&]() { return stripe_uncopied[sp].load() == 0; });
			}
			BNOTE("stripe %zu is in the pinned arena", sp);
			if (L.stripe_base[sp + 1] > L.stripe_base[sp])
				ACM_HIP_TRY(hipMemcpyAsync(d_stage + L.stripe_base[sp], h_files + L.stripe_base[sp], L.stripe_base[sp + 1] - L.stripe_base[sp],
							   hipMemcpyHostToDevice, st_up));
			ACM_HIP_TRY((hipError_t)acmk_launch_scatter_stripe(reinterpret_cast<const AcmParseJob *>(d_jobs), (uint32_t)nd,
									   reinterpret_cast<const uint64_t *>(d_jobs + L.stripe_tab_off), d_stage, d_files,
									   (uint32_t)sp, (uint32_t)R, st_up));
			ACM_HIP_TRY(hipEventRecord(ev_stripe[sp + 1], st_up));
			/* range r is walked behind stripe r + STRIPE_MARGIN: its blocks end near the end of stripe r of the bits, and how
			 * near depends on how evenly the stream spends them (a corpus of short files: a range is a block or two) */
			if (sp + 1 < R) {
				if (sp >= STRIPE_MARGIN) {
					ACM_HIP_TRY(hipStreamWaitEvent(st_parse, ev_stripe[sp + 1], 0));
					ACM_TRY(launch_range(sp - STRIPE_MARGIN, sp + 1));
				}
			} else {
				BNOTE("last stripe of the files queued for upload");
				ACM_HIP_TRY(hipStreamWaitEvent(st_parse, ev_stripe[R], 0));
				for (size_t r = R > STRIPE_MARGIN ? R - STRIPE_MARGIN - 1 : 0; r < R; r++)
					if (r + STRIPE_MARGIN + 1 >= R)         /* the ranges no earlier stripe has released */
						ACM_TRY(launch_range(r, 0));
			}
		}
	}
	ACM_HIP_TRY(hipMemcpyAsync(h_jobs + L.jobs_bytes, d_jobs + L.jobs_bytes, L.res_bytes, hipMemcpyDeviceToHost, st_parse));
	if (d_marks && L.hdr_total)             /* the marks of every range, once, behind the last range's walk */
		ACM_HIP_TRY(hipMemcpyAsync(h_marks, d_marks, L.hdr_total * sizeof(acm_block_mark), hipMemcpyDeviceToHost, st_parse));
	ACM_HIP_TRY(hipEventRecord(ev_parsed, st_parse));
	return ACMHIP_OK;
}

/* what the device parser said; the streams it flags go through the exact host reader here (block ranges: noted for the fix-up).  Waits
 * for the results queued by upload_and_walk(); does nothing the second time or without device parsing */
int BatchRun::settle()
{
	if (settled || !ev_parsed)
		return ACMHIP_OK;
	settled = true;
	if (hipEventSynchronize(ev_parsed) != hipSuccess)
		return acmhip_report_hip((int)hipGetLastError(), "device parsing");
	t_dev_parsed = clk::now();
	BNOTE("device parsing done");
	for (size_t k = 0; k < nd; k++) {
		const size_t i = L.dev_ids[k];
		Slot &s = slots[i];
		const SlotLayout &p = L.slots[i];
		if (!parse_clean(results[k], flags[k], p.need_blocks)) {
			s.pk_ntiles = 0;                /* whatever the device wrote of its byte-plane form is not to be read: the host stages int16 */
			if (R > 1) {
				redo.push_back(i);
				continue;
			}
			ACM_TRY(host_arenas(dev, L.idx_total, L.hdr_total, &h_idx, &h_hdr));
			host_stage(i);
			tm.host_parsed++;
			replan[p.chunk] = 1;
			continue;
		}
		s.info.blocks = (uint32_t)p.need_blocks;
		s.info.end_status = ACM_OK;
		items[i].status = ACM_OK;
		items[i].words = deliverable_words(s.info.total_values, (uint64_t)s.info.rows * s.info.cols, s.info.channels, p.need_blocks);
		tm.device_parsed++;
		if (index) {
			/* a clean walk: the marks it left beside the headers, and the entry behind the last block from where it ended */
			memcpy(index[i].marks, h_marks + p.hdr_off, p.need_blocks * sizeof(acm_block_mark));
			index[i].marks[p.need_blocks] = acm_block_mark{ results[k].end_bit, 0, 0 };
			index_staged(i, ACM_OK, s.info);
		}
	}
	return ACMHIP_OK;
}

/* uploads of many small pieces of one arena (a stream's byte-plane block, its int16 tail): a transfer call costs what ~256 KB cost
 * on the wire, so pieces closer together than that travel as one, the bytes between them with them (unread on the device); a
 * batch of 65 536 small streams is a few transfers per chunk instead of two per stream.  Sends `spans` and empties it */
hipError_t BatchRun::upload_spans(uint8_t *d_base, const uint8_t *h_base)
{
	constexpr uint64_t JOIN = 256u << 10;
	for (size_t k = 0; k < spans.size();) {
		uint64_t at = spans[k].at, end = spans[k].at + spans[k].len, payload = spans[k].len;
		size_t j = k + 1;
		while (j < spans.size() && spans[j].at >= at && spans[j].at <= end + JOIN) {
			end = std::max(end, spans[j].at + spans[j].len);
			payload += spans[j].len;
			j++;
		}
		const hipError_t e = hipMemcpyAsync(d_base + at, h_base + at, end - at, hipMemcpyHostToDevice, st_main);
		if (e != hipSuccess)
			return e;
		tm.h2d_bytes += std::min(payload, end - at);      /* what the plans read; the gaps a joined transfer carries along are nobody's */
		k = j;
	}
	spans.clear();
	return hipSuccess;
}

/* host parsing with a second form: the second form of the chunk (packed: the used front of its blob region and its chunk-table entries;
 * byte planes: the blocks of the streams that have one); of the int16 arena only what the other kernels read - streams without
 * a second form, and behind a stream's whole tiles its ragged tail with the two rows in front of it.  Needs the chunk's plan */
int BatchRun::upload_forms_and_tails(size_t c)
{
	const ChunkLayout &cl = L.chunks[c];
	Chunk &ch = chunks[c];
	if (L.stage_mform) {
		size_t in_plan_mf = 0;
		for (size_t i = cl.first; i < cl.last; i++) {
			const Slot &s = slots[i];
			if (!s.ok || items[i].words == 0)
				continue;
			const size_t at = in_plan_mf++;
			if (!s.pk_ntiles)
				continue;
			uint64_t rows2 = 0;
			ACM_TRY(acmhip_plan_form_rows(ch.plan, at, &rows2));
			if (!rows2)
				continue;               /* the plan reads this stream's int16 rows (see below): its byte-plane block stays here */
			spans.push_back(Span{ L.slots[i].mf_off, s.mf_used });
		}
		ACM_HIP_TRY(upload_spans(d_pkblob, h_pkblob));
		/* the chunk's pair-table entries in one piece (a few bytes per thousand samples; entries of streams without the form
		 * travel with them unread) instead of a transfer per stream */
		if (cl.mf_pair_end > cl.mf_pair_begin) {
			ACM_HIP_TRY(hipMemcpyAsync(reinterpret_cast<acmhip_mform_pair *>(d_pkchunk) + cl.mf_pair_begin,
						   reinterpret_cast<acmhip_mform_pair *>(h_pkchunk) + cl.mf_pair_begin,
						   (cl.mf_pair_end - cl.mf_pair_begin) * sizeof(acmhip_mform_pair), hipMemcpyHostToDevice, st_main));
			tm.h2d_bytes += (cl.mf_pair_end - cl.mf_pair_begin) * sizeof(acmhip_mform_pair);
		}
		tm.h2d_bytes += (cl.hdr_end - cl.hdr_begin) * sizeof(acmhip_blkhdr);
	} else {
		const uint64_t region = cl.idx_begin * sizeof(int16_t), region_len = (cl.idx_end - cl.idx_begin) * sizeof(int16_t);
		const uint64_t used = std::min<uint64_t>(ch.pk_used.load(), region_len);
		if (used)
			ACM_HIP_TRY(hipMemcpyAsync(d_pkblob + region, h_pkblob + region, used, hipMemcpyHostToDevice, st_main));
		tm.h2d_bytes += used + (cl.pk_chunk_end - cl.pk_chunk_begin) * sizeof(acmhip_packed_chunk) + (cl.hdr_end - cl.hdr_begin) * sizeof(acmhip_blkhdr);
		if (cl.pk_chunk_end > cl.pk_chunk_begin)
			ACM_HIP_TRY(hipMemcpyAsync(d_pkchunk + cl.pk_chunk_begin, h_pkchunk + cl.pk_chunk_begin,
						   (cl.pk_chunk_end - cl.pk_chunk_begin) * sizeof(acmhip_packed_chunk), hipMemcpyHostToDevice, st_main));
	}
	size_t in_plan = 0;            /* position among the descriptors build_plan() made the chunk's plan from */
	for (size_t i = cl.first; i < cl.last; i++) {
		const Slot &s = slots[i];
		if (!s.ok || items[i].words == 0)
			continue;
		const size_t at = in_plan++;
		if (s.info.blocks == 0)
			continue;
		const uint64_t cols = s.info.cols, nrows = (uint64_t)s.info.blocks * s.info.rows;
		uint64_t from_row = 0;
		if (s.pk_ntiles) {
			/* what the plan really takes from the second form - asked of the plan, not assumed: a level-13 / 14 stream of a
			 * small plan (or with ACM_PREFIX=0) goes to kernels that read the int16 rows from row 0 on */
			uint64_t rows2 = 0;
			ACM_TRY(acmhip_plan_form_rows(ch.plan, at, &rows2));
			if (s.mf_fused && rows2 != (uint64_t)s.pk_ntiles * (uint64_t)acmhip_mform_tile_rows(s.info.level)) {
				/* the parsing pass wrote only the int16 rows behind the tiles it put into the form: a plan that reads fewer of
				 * them from the form would decode rows that were never staged.  Stager and planner cut by the same tile
				 * geometry of the same library build, and the shipped build reads no kernel-selection switch from the
				 * environment any more (ACM_K1_VARIANT made the two disagree), so this is an internal error,
				 * reported as text, not a condition to recover from */
				char msg[200];
				snprintf(msg, sizeof(msg), "acm_batch_decode: stream %zu: the plan reads %llu rows from the byte-plane form, %llu were staged that way",
					 i, (unsigned long long)rows2, (unsigned long long)s.pk_ntiles * (unsigned long long)acmhip_mform_tile_rows(s.info.level));
				acmhip_set_error_text(msg);
				return ACMHIP_ERR_ARG;
			}
			if (rows2 && rows2 * cols >= items[i].words)
				continue;               /* nothing behind the whole tiles is emitted */
			from_row = rows2 >= 2 ? rows2 - 2 : 0;
		}
		spans.push_back(Span{ (L.slots[i].idx_off + from_row * cols) * sizeof(int16_t), (nrows - from_row) * cols * sizeof(int16_t) });
	}
	ACM_HIP_TRY(upload_spans(reinterpret_cast<uint8_t *>(d_idx), reinterpret_cast<const uint8_t *>(h_idx)));
	ACM_HIP_TRY(hipMemcpyAsync(d_hdr + cl.hdr_begin, h_hdr + cl.hdr_begin, (cl.hdr_end - cl.hdr_begin) * sizeof(acmhip_blkhdr),
				   hipMemcpyHostToDevice, st_main));
	return ACMHIP_OK;
}

/* host parsing, int16 only: the chunk's slices of the index and header arenas, each in one piece.  Needs the chunk parsed */
int BatchRun::upload_int16_slice(size_t c)
{
	const ChunkLayout &cl = L.chunks[c];
	tm.h2d_bytes += (cl.idx_end - cl.idx_begin) * sizeof(int16_t) + (cl.hdr_end - cl.hdr_begin) * sizeof(acmhip_blkhdr);
	ACM_HIP_TRY(hipMemcpyAsync(d_idx + cl.idx_begin, h_idx + cl.idx_begin, (cl.idx_end - cl.idx_begin) * sizeof(int16_t),
				   hipMemcpyHostToDevice, st_main));
	ACM_HIP_TRY(hipMemcpyAsync(d_hdr + cl.hdr_begin, h_hdr + cl.hdr_begin, (cl.hdr_end - cl.hdr_begin) * sizeof(acmhip_blkhdr),
				   hipMemcpyHostToDevice, st_main));
	return ACMHIP_OK;
}

/* device parsing: only what the host reader staged itself (streams the device parser did not take or gave up on).  Needs settle() */
int BatchRun::upload_host_staged(size_t c)
{
	for (size_t i = L.chunks[c].first; i < L.chunks[c].last; i++) {
		const Slot &s = slots[i];
		const SlotLayout &p = L.slots[i];
		if (!s.ok || !s.host_staged || s.info.blocks == 0)
			continue;
		const uint64_t bl = (uint64_t)s.info.rows * s.info.cols;
		ACM_HIP_TRY(hipMemcpyAsync(d_idx + p.idx_off, h_idx + p.idx_off, s.info.blocks * bl * sizeof(int16_t), hipMemcpyHostToDevice, st_main));
		ACM_HIP_TRY(hipMemcpyAsync(d_hdr + p.hdr_off, h_hdr + p.hdr_off, s.info.blocks * sizeof(acmhip_blkhdr), hipMemcpyHostToDevice, st_main));
	}
	return ACMHIP_OK;
}

/* 3. this thread feeds the device, chunk by chunk (with block ranges upload_and_walk() has queued everything already) */
int BatchRun::feed_chunks()
{
	for (size_t c = 0; c < chunks.size() && R == 1; c++) {
		const ChunkLayout &cl = L.chunks[c];
		Chunk &ch = chunks[c];
		if (ev_parsed) {
			ACM_TRY(settle());
			if (c == 0)
				ACM_HIP_TRY(hipStreamWaitEvent(st_main, ev_parsed, 0));
		}
		{
			std::unique_lock<std::mutex> g(m);
			cv.wait(g, [&]() { return ch.unparsed.load() == 0; });
		}
		if (!planned[c] || replan[c])
			ACM_TRY(build_plan(c));
		for (size_t i = cl.first; i < cl.last; i++)
			if (slots[i].ok)
				tm.samples += items[i].words;
		if (ch.plan) {
			ACM_HIP_TRY(hipEventRecord(ch.ev[0], st_main));
			if (!L.dev_parse && (L.stage_packed || L.stage_mform))
				ACM_TRY(upload_forms_and_tails(c));
			else if (!L.dev_parse)
				ACM_TRY(upload_int16_slice(c));
			else
				ACM_TRY(upload_host_staged(c));
			ACM_HIP_TRY(hipEventRecord(ch.ev[1], st_main));
			ACM_TRY(launch(ch.plan));
			ACM_HIP_TRY(hipEventRecord(ch.ev[2], st_main));
			ACM_HIP_TRY(hipStreamWaitEvent(st_copy, ch.ev[2], 0));
			ACM_HIP_TRY(hipEventRecord(ch.ev[3], st_copy));
			if (L.direct_out) {
				for (size_t i = cl.first; i < cl.last; i++) {
					if (!slots[i].ok || !items[i].pcm || items[i].words == 0)
						continue;
					const uint64_t w = std::min<uint64_t>(items[i].words, items[i].pcm_cap);
					ACM_HIP_TRY(hipMemcpyAsync(items[i].pcm, d_pcm + L.slots[i].pcm_off, w * sizeof(int16_t), hipMemcpyDeviceToHost, st_copy));
				}
			} else if (!L.keep_on_device) {
				ACM_HIP_TRY(hipMemcpyAsync(h_pcm + cl.idx_begin, d_pcm + cl.idx_begin, (cl.idx_end - cl.idx_begin) * sizeof(int16_t),
							   hipMemcpyDeviceToHost, st_copy));
			}
		}
		ACM_HIP_TRY(hipEventRecord(ch.ev[4], st_copy));
		BNOTE("chunk %zu: synthesis and read-back queued", c);
		announce(c);
	}
	return ACMHIP_OK;
}

/* everything is queued: the device parser's verdict on block ranges, the pool's end, idle streams, then the fix-up */
int BatchRun::finish()
{
	if (R > 1)
		ACM_TRY(settle());
	pool.wait();
	pool_busy = false;
	BNOTE("pool done");
	ACM_HIP_TRY(hipStreamSynchronize(st_copy));
	ACM_HIP_TRY(hipStreamSynchronize(st_main));
	if (R > 1) {
		if (!redo.empty())
			ACM_TRY(fix_up());
		for (size_t i = 0; i < n; i++)
			if (slots[i].ok)
				tm.samples += items[i].words;
	}
	return ACMHIP_OK;
}

/* fix-up (block ranges, rare): what the device parser flagged goes through the exact host reader and one more plan, stream by
 * stream in the now idle arenas; its PCM replaces whatever the ranges copied out for these streams.  Needs the pool done and the
 * streams idle */
int BatchRun::fix_up()
{
	ACM_TRY(host_arenas(dev, L.idx_total, L.hdr_total, &h_idx, &h_hdr));
	PlanStreams ps;
	std::vector<size_t> live;
	for (size_t i : redo) {
		host_stage(i);
		tm.host_parsed++;
		const Slot &s = slots[i];
		const SlotLayout &p = L.slots[i];
		if (!s.ok || items[i].words == 0 || s.info.blocks == 0)
			continue;
		const uint64_t bl = (uint64_t)s.info.rows * s.info.cols;
		ACM_HIP_TRY(hipMemcpyAsync(d_idx + p.idx_off, h_idx + p.idx_off, s.info.blocks * bl * sizeof(int16_t), hipMemcpyHostToDevice, st_main));
		ACM_HIP_TRY(hipMemcpyAsync(d_hdr + p.hdr_off, h_hdr + p.hdr_off, s.info.blocks * sizeof(acmhip_blkhdr), hipMemcpyHostToDevice, st_main));
		ps.add(s.info, p.idx_off, p.hdr_off, p.pcm_off, s.info.blocks * s.info.rows, 0, items[i].words, s.patches);
		live.push_back(i);
	}
	if (!ps.descs.empty()) {
		acmhip_plan *fix = nullptr;
		ACM_TRY(acmhip_plan_create(dev, ps.descs.data(), ps.descs.size(), ps.patches.data(), ps.patches.size(), opts.plan_flags, &fix));
		int rc = launch(fix);
		for (size_t i : live)
			if (rc == ACMHIP_OK && items[i].pcm && !out_f32) {
				const uint64_t w = std::min<uint64_t>(items[i].words, items[i].pcm_cap);
				if (hipMemcpyAsync(h_pcm + L.slots[i].pcm_off, d_pcm + L.slots[i].pcm_off, w * sizeof(int16_t), hipMemcpyDeviceToHost, st_main) != hipSuccess)
					rc = acmhip_report_hip((int)hipGetLastError(), "fix-up read-back");
			}
		if (rc == ACMHIP_OK && hipStreamSynchronize(st_main) != hipSuccess)
			rc = acmhip_report_hip((int)hipGetLastError(), "fix-up");
		acmhip_plan_destroy(fix);
		ACM_TRY(rc);
		for (size_t i : live)
			if (items[i].pcm && !out_f32)
				memcpy(items[i].pcm, h_pcm + L.slots[i].pcm_off, std::min<uint64_t>(items[i].words, items[i].pcm_cap) * sizeof(int16_t));
	}
	BNOTE("fix-up of %zu flagged streams done", redo.size());
	return ACMHIP_OK;
}

/* timing: the phases overlap; report the device-side time each one took (summed over chunks) and the wall clock.  Needs finish() */
void BatchRun::roll_up(acm_batch_timing *timing)
{
	float ms = 0;
	for (Chunk &ch : chunks) {
		if (!ch.plan)
			continue;
		if (hipEventElapsedTime(&ms, ch.ev[0], ch.ev[1]) == hipSuccess)
			tm.h2d_s += ms * 1e-3;
		if (hipEventElapsedTime(&ms, ch.ev[1], ch.ev[2]) == hipSuccess)
			tm.kernel_s += ms * 1e-3;
		if (hipEventElapsedTime(&ms, ch.ev[3], ch.ev[4]) == hipSuccess)
			tm.d2h_s += ms * 1e-3;
	}
	for (Chunk &ch : rchunks) {             /* block ranges: ev[0] .. ev[2] bracket the synthesis on the device stream */
		if (ch.plan && hipEventElapsedTime(&ms, ch.ev[0], ch.ev[2]) == hipSuccess)
			tm.kernel_s += ms * 1e-3;
		if (hipEventElapsedTime(&ms, ch.ev[3], ch.ev[4]) == hipSuccess)
			tm.d2h_s += ms * 1e-3;
	}
	double h2d_files_s = 0;
	for (size_t g = 0; g < groups.size(); g++)
		if (R == 1 && L.groups[g].k_first != L.groups[g].k_last && hipEventElapsedTime(&ms, groups[g].ev[0], groups[g].ev[1]) == hipSuccess)
			h2d_files_s += ms * 1e-3;
	/* striped upload: first stripe queued .. last stripe in place (the stripes wait for the pool's copies in between) */
	if (R > 1 && hipEventElapsedTime(&ms, ev_stripe[0], ev_stripe[R]) == hipSuccess)
		h2d_files_s = ms * 1e-3;
	tm.h2d_s += h2d_files_s;
	if (L.dev_parse)
		tm.h2d_bytes += L.files_total;
	for (const Slot &s : slots)
		tm.packed_streams += s.pk_ntiles != 0;
	/* host-side staging: headers, then until the last stream was parsed - by the pool, or by the device (whose walks
	 * overlap the uploads of the later groups and the synthesis / read-back of the earlier ones) */
	tm.stage_s = secs(t0, t_hdr) + std::max(secs(t_alloc, t_parsed), secs(t_alloc, t_dev_parsed));
	tm.total_s = secs(t0, clk::now());
	if (timing)
		*timing = tm;
}
#undef BNOTE

} // namespace

extern "C" int acm_batch_decode(acmhip_device *dev, acm_batch_item *items, size_t n,
				const acm_batch_opts *opts_in, acm_batch_timing *timing)
{
	return acm_batch_decode_indexed(dev, items, n, opts_in, nullptr, timing);
}

extern "C" int acm_batch_decode_indexed(acmhip_device *dev, acm_batch_item *items, size_t n, const acm_batch_opts *opts_in,
					acm_batch_index_out *index, acm_batch_timing *timing)
{
	if (!dev || (n && !items))
		return ACMHIP_ERR_ARG;
	acm_batch_opts opts{};
	if (opts_in)
		opts = *opts_in;
	if (opts.fmt > 3 || opts.parse > ACM_BATCH_PARSE_AUTO)
		return ACMHIP_ERR_ARG;
	/* float32 output: device-resident, the s16le samples scaled, every plan launched through acmhip_plan_launch_f32 */
	if ((opts.flags & ACM_BATCH_PCM_F32) && (!opts.d_pcm || opts.fmt != ACMHIP_FMT_S16LE || (opts.flags & ACM_BATCH_STAGE_PACKED))) {
		acmhip_set_error_text("ACM_BATCH_PCM_F32: device-resident output (opts->d_pcm), ACMHIP_FMT_S16LE and no ACM_BATCH_STAGE_PACKED");
		return ACMHIP_ERR_ARG;
	}
	/* parsed ahead of time (acm_batch_prestage): must be these very items */
	if (const acm_batch_prestaged *pre = opts.prestaged) {
		if (pre->items.size() != n || pre->force_chans != opts.force_chans)
			return ACMHIP_ERR_ARG;
		for (size_t i = 0; i < n; i++)
			if (pre->data[i] != items[i].data || pre->len[i] != items[i].len)
				return ACMHIP_ERR_ARG;          /* the staged blocks are copied into arenas laid out from THESE items' lengths */
	}
	const auto t0 = clk::now();
	const int threads_wanted = opts.threads > 0 ? opts.threads : default_threads();
	Pool pool((int)std::min<size_t>((size_t)threads_wanted, std::max<size_t>(1, n)));

	/* 1. headers -> the layout: where everything goes and which way every stream travels (acm_batch_layout.cpp) */
	std::vector<LayoutItem> probed(n);
	if (index) {
		/* room for every item's whole index, checked before anything is written: items, PCM and marks stay as they are */
		std::vector<uint8_t> short_of(n, 0);
		pool.run(n, [&](size_t i) {
			acm_stage_info info;
			short_of[i] = acm_stage_probe(items[i].data, items[i].len, opts.force_chans, &info) == ACM_OK &&
				      (!index[i].marks || index[i].max_blocks < blocks_possible(info, items[i].len));
		});
		for (size_t i = 0; i < n; i++)
			if (short_of[i]) {
				acmhip_set_error_text("acm_batch_decode_indexed: an item's marks are missing or hold fewer than acm_batch_index_blocks() asks for");
				return ACMHIP_ERR_ARG;
			}
	}
	pool.run(n, [&](size_t i) {
		acm_batch_item &it = items[i];
		acm_stage_info &info = probed[i].info;
		it.words = 0;
		it.dev_off = 0;
		it.status = acm_stage_probe(it.data, it.len, opts.force_chans, &info);
		if (index) {                            /* a file that is not ACM: acm_index_file's answer, its marks untouched */
			index[i].status = (index[i].marks || it.status == ACMHIP_ERR_ARG) ? it.status : ACMHIP_ERR_ARG;
			index[i].blocks = 0;
			index[i].end_status = 0;
		}
		it.level = info.level;
		it.rows = info.rows;
		it.channels = info.channels;
		it.rate = info.rate;
		it.total_values = info.total_values;
		probed[i].len = it.len;
		probed[i].ok = (it.status == ACM_OK);
		probed[i].has_pcm = it.pcm != nullptr;
	});
	BatchLayout layout;
	ACM_TRY(acm_batch_layout(probed.data(), n, opts, threads_wanted, opts.prestaged != nullptr, &layout));
	for (size_t i = 0; i < n; i++)
		items[i].dev_off = layout.slots[i].pcm_off;

	BatchRun run(dev, items, n, opts, layout, pool, probed, index, t0, clk::now());
	ACM_TRY(run.acquire());                 /* arenas, streams, events */
	ACM_TRY(run.start_pool());              /* 2a / 2b. the device parser's tables; the pool: file copies, host parsing, copy-out */
	ACM_TRY(run.plan_device_chunks());
	ACM_TRY(run.upload_and_walk());         /* 2c. files up, the walk behind them (block ranges: all of the batch, range by range) */
	ACM_TRY(run.feed_chunks());             /* 3. feed the device, chunk by chunk */
	ACM_TRY(run.finish());                  /* the pool's end, idle streams, fix-up */
	run.roll_up(timing);                    /* timing */
	return ACMHIP_OK;
}
