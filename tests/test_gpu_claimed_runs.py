"""The chunk kernel's claimed runs (libacm_amd/csrc/acm_kernels.hip: acm_chunk, acmk_tile2m_split), bit-exact against the CPU oracle.

A launch's chunk table is handed out as one static run per wavefront plus, behind them, runs of run_chunks chunks that the wavefronts
claim with an atomic increment as they come free.  The compiled-in policy only splits tables of 32 chunks per wavefront and more;
acmk_tile2m_claim_config puts a policy in force for small tables, and every case here uses it - and restores the default in a
`finally` - to reach, with tables of three chunks per wavefront, what can go wrong: claimed runs of two and three chunks (the records
asked for two and three chunks ahead lie behind the run's end), a last claimed run of one chunk, a single claimed run, fewer runs than
wavefronts, runs that start at a stream's first chunk, inside a stream (the chunk in front is replayed) and at a window's lead-in
record, the claim word left at zero by every launch (launches back to back, a captured launch replayed), big-endian unsigned output
and the float32 twin.  The batches, their oracle PCM and the checking are tests/test_gpu_long_runs.py's: the PCM arena is poisoned
in front of every launch that is checked."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import helpers  # noqa: F401  (GPU tests run with the fill mode on: helpers sets the switch)
from libacm_amd import capi
from test_gpu_long_runs import Batch, L, cus, launch_and_check, lean_layout, lean_where, release

pytestmark = pytest.mark.gpu


def claim_lib():
    lib = L()
    lib.acmk_tile2m_split.argtypes = [C.c_uint32, C.c_int, C.c_uint32] + [C.POINTER(C.c_uint32)] * 3
    lib.acmk_tile2m_claim_config.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.acmk_tile2m_claim_config.restype = None
    return lib


@contextlib.contextmanager
def policy(run_chunks, permille):
    lib = claim_lib()
    lib.acmk_tile2m_claim_config(run_chunks, permille, None, None)
    try:
        yield
    finally:
        lib.acmk_tile2m_claim_config(-1, -1, None, None)


def split(level, n):
    """(static_per, run_chunks, nclaimed) of a table of n chunks under the policy in force"""
    sp, rc, nc = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert claim_lib().acmk_tile2m_split(level, cus(), n, C.byref(sp), C.byref(rc), C.byref(nc)) == 0
    return sp.value, rc.value, nc.value


class Rig:
    """a batch of 3 W chunks at one level, staged, uploaded (room for float32 PCM), with its plan on the byte-plane form"""

    def __init__(self, dev, level):
        Lb = L()
        self.level = level
        self.T2, self.T2M, self.W = Lb.acmk_tile2_rows(level), Lb.acmk_tile2m_rows(level), Lb.acmk_tile2m_run_waves(level, cus())
        q = self.T2 // self.T2M
        assert self.W > 0 and (3 * self.W) % q == 0 and Lb.acmk_tile2m_stages(level) == 6
        self.b = Batch(level, self.T2, 3 * self.W // q, 130000 + 1000 * level, self.T2M)
        self.bases, self.N = lean_layout(self.b, self.T2, self.T2M)
        assert self.N == 3 * self.W
        self.mf = self.b.mform()
        self.plans, self.ptrs = [], []
        self.dev = dev
        self.ptrs = self.b.upload(dev, self.b.ar.pcm_words) + list(self.mf.upload(dev))
        self.plan = self.new_plan(dev)

    def new_plan(self, dev):
        plan = capi.Plan(dev, self.b.descs, self.b.ar.patches, packed=self.mf.streams)
        self.plans.append(plan)
        assert plan.stats().mform_tiles == self.N
        plan.bind_mform(*self.ptrs[3:])
        return plan

    def check(self, plan, what, fmt=capi.FMT_S16LE):
        launch_and_check(self.dev, self.b, plan, self.ptrs, what, fmt=fmt, where=lean_where(self.bases, self.T2M, self.W, self.N))

    def close(self):
        release(self.dev, self.plans, self.ptrs)


@pytest.fixture(scope="module")
def rigs(dev):
    made = {}

    def get(level):
        if level not in made:
            made[level] = Rig(dev, level)
        return made[level]
    yield get
    for r in made.values():
        r.close()


@pytest.mark.parametrize("run_chunks", [2, 3])
@pytest.mark.parametrize("level", [9, 8, 11])
def test_whole_table_claimed(rigs, level, run_chunks):
    """no static runs at all: every wavefront claims its first run on entry, and every run it ever has is two or three chunks long.
    Level 9: two walkers, history handed over by DPP; 8: four walkers; 11: chunks of one row, history in registers"""
    r = rigs(level)
    with policy(run_chunks, 0):
        assert split(level, r.N) == (0, run_chunks, -(-r.N // run_chunks))
        r.check(r.plan, "acm_chunk, the whole table in claimed runs of %d" % run_chunks)


@pytest.mark.parametrize("run_chunks,nclaimed,last", [(3, None, 1), (None, 1, None), (16, None, None)])
def test_static_runs_of_two_then_claimed_runs(rigs, run_chunks, nclaimed, last):
    """static runs of two chunks, the third W chunks claimed: in runs of three, the last of which holds one chunk; as ONE claimed run;
    in runs of sixteen - far fewer runs than wavefronts, most of which are refused at their first claim"""
    r = rigs(9)
    rc = run_chunks or r.W
    with policy(rc, 700):
        sp, got_rc, nc = split(9, r.N)
        assert (sp, got_rc, nc) == (2, rc, -(-r.W // rc)) and nc < r.W
        if nclaimed is not None:
            assert nc == nclaimed
        if last is not None:
            assert r.N - 2 * r.W - (nc - 1) * rc == last
        r.check(r.plan, "acm_chunk, static runs of 2 + %d claimed runs of %d" % (nc, rc))


@pytest.mark.parametrize("level", [9, 11])
def test_claimed_runs_start_everywhere(dev, rigs, level):
    """a plan with windows into the batch's streams behind the whole streams (as test_chunk_kernel_long_runs builds it), the second half
    of its table claimed in runs of three: claimed runs start at a stream's first chunk (ACM_TILE_FRESH: nothing replayed), inside a
    stream (the chunk in front is replayed into the sink) and at a window's ACM_TILE_DISCARD lead-in record - asserted from the layout"""
    r = rigs(level)
    b, T2, T2M, W, n = r.b, r.T2, r.T2M, r.W, len(r.b.descs)
    cols = 1 << level
    nl = min(T2 // T2M, L().acmk_tile2m_lead_in(level))
    wins = [(k, (1 + k % (b.whole_rows(k) // T2 - 1)) * T2) for k in range(n) if not b.h1[k] and b.whole_rows(k) // T2 >= 2][:96]
    assert len(wins) > 40
    wdescs, at = [], b.ar.pcm_words
    for k, rb in wins:
        d = b.descs[k]
        ne = d.n_emit - rb * cols
        wdescs.append(capi.StreamDesc(idx_off=d.idx_off, hdr_off=d.hdr_off, pcm_off=at, n_emit=ne, level=level, rows=d.rows, nrows=d.nrows,
                                      row_begin=rb))
        at += (ne + 63) // 64 * 64
    descs2, src2 = list(b.descs) + wdescs, list(range(n)) + [k for k, _ in wins]
    wb, N2 = lean_layout(b, T2, T2M, descs2, src2, lead=nl)
    fresh, lead_in = set(), set()
    for d, base in zip(descs2, wb):
        if base is None:
            continue
        if d.row_begin:
            lead_in.update(range(base[1] - nl, base[1]))
        else:
            fresh.add(base[1])
    plans, ptrs = [], []
    try:
        with policy(3, 500):
            sp, rc, nc = split(level, N2)
            assert sp >= 1 and rc == 3 and nc > W // 3
            starts = [W * sp + k * rc for k in range(nc)]
            kinds = ["fresh" if s in fresh else "lead-in" if s in lead_in else "inside" for s in starts]
            assert kinds.count("fresh") >= 3 and kinds.count("lead-in") >= 3 and kinds.count("inside") >= 3, (
                kinds.count("fresh"), kinds.count("lead-in"), kinds.count("inside"))
            ptrs = b.upload(dev, at - b.ar.pcm_words)
            wplan = capi.Plan(dev, descs2, b.ar.patches, packed=list(r.mf.streams) + [r.mf.streams[k] for k, _ in wins])
            plans.append(wplan)
            assert wplan.stats().mform_tiles == N2, (wplan.stats().mform_tiles, N2)
            wplan.bind_mform(*r.ptrs[3:])
            launch_and_check(dev, b, wplan, ptrs, "acm_chunk with windows, claimed runs of 3", descs=descs2, src=src2,
                             where=lean_where(wb, T2M, W, N2), total_words=at)
    finally:
        release(dev, plans, ptrs)


class Times:
    """a plan launched n times back to back, nothing waited for in between"""

    def __init__(self, plan, n):
        self.plan, self.n = plan, n

    def launch(self, *a):
        for _ in range(self.n):
            self.plan.launch(*a)


def test_every_launch_leaves_the_claim_word_at_zero(rigs):
    """three launches of one plan back to back without a sync; then, over a poisoned arena, one more: a launch that found the word
    anywhere but at zero would skip runs, and the poison would show"""
    r = rigs(9)
    with policy(3, 700):
        assert split(9, r.N)[2] > 0
        r.check(Times(r.plan, 3), "acm_chunk, three launches back to back")
        r.check(r.plan, "acm_chunk, the launch behind them")
        r.check(Times(r.plan, 2), "acm_chunk, two more")


def test_a_captured_launch_replays(rigs):
    """the same for a launch captured once into a graph (torch's, on a stream of torch's) and replayed twice, the arena poisoned in
    front of each replay: nothing outside the kernel re-arms the claim word"""
    import torch
    r = rigs(9)
    dev = r.dev
    side = torch.cuda.Stream()
    d2 = plan = None
    try:
        with policy(3, 700):
            assert split(9, r.N)[2] > 0
            with torch.cuda.stream(side):
                d2 = capi.Device(0, side.cuda_stream)
                plan = capi.Plan(d2, r.b.descs, r.b.ar.patches, packed=r.mf.streams)
                plan.bind_mform(*r.ptrs[3:])
                plan.launch(*r.ptrs[:3])                # (module load and the plan's uploads: outside the capture)
                side.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    plan.launch(*r.ptrs[:3])

                class Replay:
                    def launch(self, *a):
                        dev.sync()                      # (the poison is queued on the session handle's stream)
                        g.replay()
                        side.synchronize()
                for k in range(2):
                    r.check(Replay(), "acm_chunk, replay %d of a captured launch" % (k + 1))
    finally:
        if plan is not None:
            plan.destroy()
        if d2 is not None:
            d2.close()


def test_u16be(rigs):
    r = rigs(9)
    with policy(3, 700):
        assert split(9, r.N)[2] > 0
        r.check(r.plan, "acm_chunk U16BE, claimed runs of 3", fmt=capi.FMT_U16BE)


def test_float32_twin(rigs):
    """acmhip_plan_launch_f32 (acm_f32_chunk, the same source): every float is the s16le sample times 2^-15, in bits"""
    r = rigs(11)
    b, dev, words = r.b, r.dev, r.b.ar.pcm_words
    with policy(2, 700):
        assert split(11, r.N)[2] > 0
        dev.memset(r.ptrs[2], 0xA5, 4 * words)
        r.plan.launch_f32(*r.ptrs[:3])
        dev.sync()
    got = np.empty(words, dtype=np.float32)
    dev.download(got, r.ptrs[2])
    bad = []
    for k, d in enumerate(b.descs):
        g = got[d.pcm_off:d.pcm_off + d.n_emit].view(np.uint32)
        w = (b.want[k].view(np.int16).astype(np.float32) / np.float32(32768)).view(np.uint32)
        if not np.array_equal(g, w):
            bad.append("stream %d: %d of %d samples differ, first at %d" % (k, int((g != w).sum()), d.n_emit, int(np.nonzero(g != w)[0][0])))
    assert not bad, "acm_f32_chunk, claimed runs of 2: %d streams differ\n  %s" % (len(bad), "\n  ".join(bad[:10]))
