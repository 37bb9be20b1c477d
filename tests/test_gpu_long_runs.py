"""Parity of the persistent kernels PAST the first record of each run, against the CPU oracle, bit-exact.

Every lean kernel splits its record table into one contiguous run per workgroup (per wavefront for acm_chunk), of ceil(records /
slots) records each (libacm_amd/csrc/acm_kernels.hip: acm_chunk, acm_tile2 / tile2m / tile2p, acm_fused_tile in carry mode).  A
batch smaller than one record per slot gives runs of ONE record, and the code that only runs from a run's second record on - the
chunk kernel's history rows in registers or handed over by DPP, its fast paths, the carries between tiles, a FRESH record or a
window's ACM_TILE_DISCARD lead-in records after another stream's record - is not reached.  Each batch here is sized from the live
geometry (the device's CU count, the kernels' exported grid and tile sizes) so that every run of the kernel under test holds at
least RUN_MIN records, which is asserted from the plan's own record counts; it mixes long streams with streams of one or two tiles
(FRESH records inside runs), block heights around the chunk's rows, every width class of the byte-plane form and a few H1-patched
streams (which leave the lean tables, so that their neighbours meet inside a run).  Every stream's PCM is compared in full with
the oracle's (reference semantics: decode.c:580-677 per stream), the PCM arena poisoned with 0xA5 in front of every launch; a
difference is reported with its stream, first sample, record and the record's place in its run.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import helpers  # noqa: F401  (GPU tests run with the fill mode on: helpers sets the switch)
import oracle_api as O
from libacm_amd import capi, synth, workload

pytestmark = pytest.mark.gpu

RUN_MIN = 6
THREADS = max(1, min(32, workload.usable_cpus()))

# content recipes, cycled over a batch: the byte-plane form's width classes throughout, and mixtures of them
RECIPES = [
    ("8 bits", dict(pwr_min=3, pwr_max=7)),
    ("12 bits", dict(pwr_min=8, pwr_max=10)),
    ("16 bits", dict(pwr_min=12, pwr_max=14)),
    ("whole range", dict(mix=synth.MIX_SINGLE, single_code=16, pwr_min=15, pwr_max=15)),
    ("mixed", dict(pwr_min=5, pwr_max=15)),
    ("val 65535", dict(pwr_min=6, pwr_max=12, val_max=65535)),
]
H1 = ("H1 patched", dict(mix=synth.MIX_UNIFORM, allow_out_of_range=1, prime_table=1, pwr_min=0, pwr_max=6))
# stream lengths in units (whole tiles of the kernel under test), with or without a ragged tail: short streams put FRESH records
# inside runs, long ones span many runs
LENGTHS = [(1, 0), (2, 0), (1, 1), (40, 1), (1, 0), (3, 1), (2, 1), (90, 0), (1, 1), (2, 0), (17, 1)]


def L():
    return capi.lib()


_cus = None


def cus():
    """the CU count the library reads (hipDeviceProp.multiProcessorCount): the grids below are sized from it"""
    global _cus
    if _cus is None:
        import torch
        _cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert _cus > 0
    return _cus


def runs(n, slots):
    """lengths of the non-empty runs when n records are split into contiguous runs of ceil(n / slots)"""
    if n == 0:
        return []
    per = -(-n // slots)
    return [min(per, n - k * per) for k in range((n + per - 1) // per)]


def min_run(n, slots):
    r = runs(n, slots)
    return min(r) if r else 0


def heights(m):
    """block heights around a chunk of m rows: 1, odd ones, exactly m, 2 m and 3 m (ACM_TILE_ONEBLOCK chunks beside general ones)"""
    return [1, 3, m, 2 * m, 5, 3 * m, 7]


class Batch:
    """streams staged into one arena, with the oracle's PCM of each"""

    def __init__(self, level, unit_rows, units, seed, m, h1_every=37, stereo_every=9, recipes=RECIPES, lengths=LENGTHS):
        """units: exact number of whole units (unit_rows rows each) over the streams that are not H1-patched"""
        cols = 1 << level
        specs, left, i = [], units, 0
        while left > 0:
            if h1_every and i % h1_every == h1_every - 1:
                recipe, n_units, tail = H1, 1 + i % 3, 1
            else:
                recipe = recipes[i % len(recipes)]
                n_units, tail = lengths[i % len(lengths)]
                n_units = min(n_units, left)
                left -= n_units
            rows = heights(m)[i % 7]
            tail_rows = (1 + (i * 7) % (unit_rows - 1)) if tail and unit_rows > 1 else 0
            cut = (1 + (i * 13) % (cols - 2)) if tail else 0
            ch = 2 if stereo_every and i % stereo_every == 3 and not cut % 2 else 1
            nr = n_units * unit_rows + tail_rows + (1 if cut else 0)
            if recipe is H1:
                nr = max(nr, 4 * rows)                  # (enough blocks for a patch to be all but certain)
            specs.append(dict(level=level, rows=rows, nblocks=-(-nr // rows), total_values=nr * cols - cut, channels=ch,
                              seed=synth.BASE_SEED + seed + i, recipe=recipe[0], **recipe[1]))
            i += 1

        def one(sp):
            kw = {k: v for k, v in sp.items() if k != "recipe"}
            f = synth.generate(**kw)
            s = capi.stage_file(f)
            want, _ = O.Oracle.decode_all(f)
            return s, want.view(np.uint16)
        with ThreadPoolExecutor(max_workers=THREADS) as ex:
            got = list(ex.map(one, specs))
        self.level, self.specs = level, specs
        self.staged = [g[0] for g in got]
        self.want = [g[1] for g in got]
        self.h1 = [s.patches is not None and len(s.patches) > 0 for s in self.staged]
        assert all(h == (sp["recipe"] == H1[0]) for h, sp in zip(self.h1, specs)), "an H1 patch where none was asked for, or none where one was"
        self.ar = capi.Arena(self.staged)
        self.descs = self.ar.descs
        for d, w in zip(self.descs, self.want):
            assert d.n_emit == w.size
        self.patch_rows = [sorted({int(p.sample) >> level for p in s.patches}) if h else None for s, h in zip(self.staged, self.h1)]
        self.units = sum(self.whole_rows(k) // unit_rows for k in range(len(specs)) if not self.h1[k])
        assert self.units == units, (self.units, units)

    def whole_rows(self, k, row_begin=0):
        d = self.descs[k]
        return min(d.nrows, d.n_emit >> d.level) - row_begin

    def upload(self, dev, extra_pcm_words=0):
        ptrs = [dev.malloc(self.ar.idx.nbytes), dev.malloc(self.ar.hdr.nbytes), dev.malloc(2 * (self.ar.pcm_words + extra_pcm_words))]
        dev.upload(ptrs[0], self.ar.idx)
        dev.upload(ptrs[1], self.ar.hdr)
        return ptrs

    def mform(self):
        mf = capi.mform_streams(self.ar.idx, self.descs, threads=THREADS)
        for k, h in enumerate(self.h1):
            if h:
                mf.streams[k].ntiles = 0
        return mf


def fused_counts(b, k):
    """records of stream k in acm_fused_tile's tables (acm_hip_api.cpp): (halo tiles, carry tiles, the clean tiles of an H1-patched
    stream, which keep the halo flavour)"""
    d = b.descs[k]
    T = L().acmk_fused_tile_rows(d.level, 0) - 2
    emit_rows = (d.n_emit + (1 << d.level) - 1) >> d.level
    if not b.h1[k]:
        return -(-emit_rows // T), -(-emit_rows // (T + 2)), 0
    pr = b.patch_rows[k]
    clean = sum(1 for r in range(0, emit_rows, T) if not any(max(r - 2, 0) <= p < min(r + T, d.nrows) for p in pr))
    return 0, 0, clean


def launch_and_check(dev, b, plan, ptrs, what, descs=None, src=None, fmt=capi.FMT_S16LE, where=None, total_words=None):
    """poison the PCM arena, launch, compare every stream of `descs` (default: the batch's; src[k]: the batch stream desc k is a window
    into) with the oracle's PCM from the desc's row_begin on"""
    descs = descs if descs is not None else b.descs
    src = src if src is not None else range(len(descs))
    words = total_words or b.ar.pcm_words
    dev.memset(ptrs[2], 0xA5, 2 * words)
    plan.launch(ptrs[0], ptrs[1], ptrs[2], fmt)
    dev.sync()
    got = np.empty(words, dtype=np.uint16)
    dev.download(got, ptrs[2])
    be, sg = (fmt & 1), not (fmt & 2)
    bad = []
    for k, (d, i) in enumerate(zip(descs, src)):
        g = got[d.pcm_off:d.pcm_off + d.n_emit]
        w = b.want[i][d.row_begin << d.level:]
        if not sg:
            w = w ^ np.uint16(0x8000)
        if be:
            w = w.byteswap()
        if not np.array_equal(g, w):
            j = int(np.nonzero(g != w)[0][0])
            row = d.row_begin + (j >> d.level)
            sp = b.specs[i]
            bad.append("desc %d = stream %d (%s, rows %d, row_begin %d): %d of %d samples differ, first at %d (row %d)%s" % (
                k, i, sp["recipe"], d.rows, d.row_begin, int((g != w).sum()), d.n_emit, j, row, where(k, row) if where else ""))
    assert not bad, "%s, level %d: %d streams differ\n  %s" % (what, b.level, len(bad), "\n  ".join(bad[:10]))


def lean_where(bases, unit, slots, nrec):
    """-> where(k, row): the record of a table split into runs over `slots` that holds row `row` of desc k (bases[k]: (the desc's first
    row on this kernel, its first record there), None: not on it), and the record's place in its run"""
    per = -(-nrec // slots)

    def where(k, row):
        if bases[k] is None:
            return " (not on this kernel)"
        r0, base = bases[k]
        t = base + (row - r0) // unit
        if t >= nrec:
            return " (behind the table)"
        return " - record %d of %d, run %d, position %d of %d" % (t, nrec, t // per, t - (t // per) * per, min(per, nrec - (t // per) * per))
    return where


def lean_layout(b, T2, unit, descs=None, src=None, lead=0):
    """(bases for lean_where, records) of the table acm_hip_api.cpp's cut_lean makes of the descs, in order: rows2 = whole tiles of T2
    rows from row_begin on in records of `unit` rows, behind `lead` lead-in records where row_begin > 0"""
    descs = descs if descs is not None else b.descs
    src = src if src is not None else range(len(descs))
    bases, n = [], 0
    for d, i in zip(descs, src):
        rows2 = b.whole_rows(i, d.row_begin) // T2 * T2
        if b.h1[i] or rows2 == 0:
            bases.append(None)
            continue
        n += lead if d.row_begin else 0
        bases.append((d.row_begin, n))
        n += rows2 // unit
    return bases, n


def table_layout(counts):
    """bases for lean_where of a table with counts[k] records of desc k (None: not in it), from the desc's row 0 on"""
    bases, n = [], 0
    for c in counts:
        bases.append(None if c is None else (0, n))
        n += c or 0
    return bases


def subset(b, keep):
    """the first `keep` streams of the batch: descs and their H1 patches"""
    pl = [p for p in b.ar.patch_list if p.stream < keep]
    return b.descs[:keep], ((capi.Patch * len(pl))(*pl) if pl else None)


def size_units(tables):
    """the least number of units for which every table - (slots, records per unit) - is split into runs of >= RUN_MIN records"""
    u = max(-(-RUN_MIN * s // r) for s, r in tables)
    while not all(min_run(u * r, s) >= RUN_MIN for s, r in tables):
        u += 1
    return u


def fit(counts, slots, base=0):
    """how many of the entries (records counts[k] each, behind `base` records) to keep so that every run holds >= RUN_MIN records"""
    keep = len(counts)
    while keep > 0 and min_run(base + sum(counts[:keep]), slots) < RUN_MIN:
        keep -= 1
    assert keep > 0 and min_run(base + sum(counts[:keep]), slots) >= RUN_MIN
    return keep


def release(dev, plans, ptrs):
    for p in plans:
        p.destroy()
    for p in ptrs:
        dev.free(p)


@pytest.mark.parametrize("level", [8, 9, 10, 11, 12])
def test_chunk_kernel_long_runs(dev, level):
    """acm_chunk (levels 8-12, byte-plane form, default flags): every wavefront's run holds >= RUN_MIN chunks - S16LE and U16BE -; the
    same plan without the form (acm_tile2 on the int16 twins, runs of >= RUN_MIN tiles); a second plan with windows into many of the
    streams from a tile boundary on (their ACM_TILE_DISCARD lead-in chunks follow another stream's chunk inside a run); at two levels
    the general tile kernel alone, halo tiles and carry runs"""
    Lb = L()
    T2, T2M = Lb.acmk_tile2_rows(level), Lb.acmk_tile2m_rows(level)
    W, G2 = Lb.acmk_tile2m_run_waves(level, cus()), Lb.acmk_tile2_grid(level, cus())
    assert T2 > 0 and T2M > 0 and T2 % T2M == 0 and W > 0 and G2 > 0
    assert Lb.acmk_tile2m_stages(level) == 6 and Lb.acmhip_mform_tile_rows(level) == T2M
    q, cols, T = T2 // T2M, 1 << level, Lb.acmk_fused_tile_rows(level, 0) - 2
    units = size_units([(W, q), (G2, 1)])
    b = Batch(level, T2, units, 60000 + 1000 * level, T2M)
    n = len(b.descs)
    mf = b.mform()
    # the mixture is there: pairs of every width class (12 bits, 8 bits, 16 bits, whole range), and adjacent chunks of one stream whose
    # first pairs differ in width
    cc = mf.class_counts()
    assert cc[0] > 32 and cc[1] > 0 and cc[2] > 0 and cc[3] > 0, cc            # (class 0 counts the table's 32 entries of slack too)
    changes = 0
    for s in mf.streams:
        if s.ntiles > 1:
            cls = mf.pairs[s.chunk_off + 1 + (np.arange(s.ntiles) * T2M) // 2] & 3
            changes += int((cls[1:] != cls[:-1]).sum())
    assert changes > 50, changes
    bases, N = lean_layout(b, T2, T2M)
    assert N == units * q and min_run(N, W) >= RUN_MIN and min_run(units, G2) >= RUN_MIN, (N, W, G2)
    rest = sum(-(-max(0, ((b.descs[k].n_emit + cols - 1) >> level) - b.whole_rows(k) // T2 * T2) // T) for k in range(n) if not b.h1[k])
    extra = sum(fused_counts(b, k)[2] for k in range(n))

    # windows into the clean streams of two tiles or more, from row k T2 (k >= 1) to the stream's end, behind all the whole streams
    nl = min(q, Lb.acmk_tile2m_lead_in(level))
    cand = [(k, (1 + k % (b.whole_rows(k) // T2 - 1)) * T2) for k in range(n) if not b.h1[k] and b.whole_rows(k) // T2 >= 2]
    wrec = [nl + b.whole_rows(k, rb) // T2 * T2 // T2M for k, rb in cand]
    wins = cand[:fit(wrec, W, N)]
    assert len(wins) > 50
    wdescs, at = [], b.ar.pcm_words
    for k, rb in wins:
        d = b.descs[k]
        ne = d.n_emit - rb * cols
        wdescs.append(capi.StreamDesc(idx_off=d.idx_off, hdr_off=d.hdr_off, pcm_off=at, n_emit=ne, level=level, rows=d.rows, nrows=d.nrows,
                                      row_begin=rb))
        at += (ne + 63) // 64 * 64
    descs2, src2 = list(b.descs) + wdescs, list(range(n)) + [k for k, _ in wins]
    wb, N2 = lean_layout(b, T2, T2M, descs2, src2, lead=nl)
    assert N2 == N + sum(wrec[:len(wins)]) and min_run(N2, W) >= RUN_MIN

    plans, ptrs = [], []
    try:
        ptrs = b.upload(dev, at - b.ar.pcm_words) + list(mf.upload(dev))
        plan = capi.Plan(dev, b.descs, b.ar.patches, packed=mf.streams)
        plans.append(plan)
        st = plan.stats()
        assert st.mform_tiles == N and st.tiles == N + rest + extra and st.stagewise_streams == 0, (st.mform_tiles, st.tiles, N, rest, extra)
        where = lean_where(bases, T2M, W, N)
        plan.bind_mform(*ptrs[3:])
        launch_and_check(dev, b, plan, ptrs, "acm_chunk", where=where)
        launch_and_check(dev, b, plan, ptrs, "acm_chunk U16BE", fmt=capi.FMT_U16BE, where=where)
        plan.bind_mform(None, None)
        launch_and_check(dev, b, plan, ptrs, "acm_tile2 on the int16 twins", where=lean_where(bases, T2, G2, units))

        wplan = capi.Plan(dev, descs2, b.ar.patches, packed=list(mf.streams) + [mf.streams[k] for k, _ in wins])
        plans.append(wplan)
        for j, (k, rb) in enumerate(wins):
            assert wplan.form_rows(n + j) == b.whole_rows(k, rb) // T2 * T2, (k, rb)        # on the lean kernels
        assert wplan.stats().mform_tiles == N2, (wplan.stats().mform_tiles, N2)
        wplan.bind_mform(*ptrs[3:])
        launch_and_check(dev, b, wplan, ptrs, "acm_chunk with windows", descs=descs2, src=src2, where=lean_where(wb, T2M, W, N2), total_words=at)

        if level in (9, 11):
            G1 = Lb.acmk_fused_grid(level, 0, cus())
            cnt = [fused_counts(b, k) for k in range(n)]
            keep = fit([c[1] for c in cnt], G1)
            descs, patches = subset(b, keep)
            halo, carry, ex = (sum(c[j] for c in cnt[:keep]) for j in range(3))
            for flags, ntab in ((capi.PLAN_NO_LEAN | capi.PLAN_FORCE_HALO, halo), (capi.PLAN_NO_LEAN | capi.PLAN_FORCE_CARRY, carry)):
                p = capi.Plan(dev, descs, patches, flags=flags)
                plans.append(p)
                stf = p.stats()
                assert stf.tiles == ntab + ex and stf.mform_tiles == 0, (flags, stf.tiles, ntab, ex)
                where = None
                if flags & capi.PLAN_FORCE_CARRY:
                    where = lean_where(table_layout([None if b.h1[k] else cnt[k][1] for k in range(keep)]), T + 2, G1, carry)
                launch_and_check(dev, b, p, ptrs, "acm_fused_tile, flags 0x%x" % flags, descs=descs, where=where)
    finally:
        release(dev, plans, ptrs)


@pytest.mark.parametrize("level,per", [(9, 2), (9, 3), (11, 2), (11, 3)])
def test_chunk_kernel_runs_of_two_and_three(dev, level, per):
    """runs of exactly two and three chunks: the records a wavefront asks for two and three chunks ahead lie behind its run's end
    (record_at names the run's last record instead)"""
    Lb = L()
    T2, T2M, W = Lb.acmk_tile2_rows(level), Lb.acmk_tile2m_rows(level), Lb.acmk_tile2m_run_waves(level, cus())
    q = T2 // T2M
    assert W > 0 and (per * W) % q == 0
    b = Batch(level, T2, per * W // q, 70000 + 1000 * level + 100 * per, T2M)
    bases, N = lean_layout(b, T2, T2M)
    assert N == per * W and set(runs(N, W)) == {per}
    mf = b.mform()
    plans, ptrs = [], []
    try:
        ptrs = b.upload(dev) + list(mf.upload(dev))
        plan = capi.Plan(dev, b.descs, b.ar.patches, packed=mf.streams)
        plans.append(plan)
        assert plan.stats().mform_tiles == N
        plan.bind_mform(*ptrs[3:])
        launch_and_check(dev, b, plan, ptrs, "acm_chunk, runs of %d" % per, where=lean_where(bases, T2M, W, N))
    finally:
        release(dev, plans, ptrs)


@pytest.mark.parametrize("level", [7, 13, 14])
def test_tile_kernel_byteplane_long_runs(dev, level):
    """acm_tile2's matrix-core builds on the byte-plane form with default flags (level 7: three stages; 13 / 14: FirstPassZW, the chunk
    kernel's six-stage first pass shared by a workgroup - a batch above the planner's own threshold for the lean kernel there), runs of
    >= RUN_MIN tiles, S16LE and U16BE; then the same plan on the int16 form"""
    Lb = L()
    T2, T2M = Lb.acmk_tile2_rows(level), Lb.acmk_tile2m_rows(level)
    GM, G2 = Lb.acmk_tile2m_grid(level, cus()), Lb.acmk_tile2_grid(level, cus())
    assert T2 > 0 and T2M > 0 and T2 % T2M == 0 and GM > 0 and G2 > 0 and Lb.acmhip_mform_tile_rows(level) == T2M
    q = T2 // T2M
    units = size_units([(GM, q), (G2, 1)])
    if level >= 13:
        units = max(units, 8 * G2)                  # (acm_hip_api.cpp: the lean kernel takes levels 13 / 14 from 8 tiles per workgroup on)
    b = Batch(level, T2, units, 80000 + 1000 * level, max(T2M, 2))
    mf = b.mform()
    cc = mf.class_counts()
    assert cc[2] > 0 and cc[3] > 0 and (level == 7 or cc[0] > 32), cc
    bases, N = lean_layout(b, T2, T2M)
    assert N == units * q and min_run(N, GM) >= RUN_MIN and min_run(units, G2) >= RUN_MIN
    plans, ptrs = [], []
    try:
        ptrs = b.upload(dev) + list(mf.upload(dev))
        plan = capi.Plan(dev, b.descs, b.ar.patches, packed=mf.streams)
        plans.append(plan)
        assert plan.stats().mform_tiles == N, (plan.stats().mform_tiles, N)
        where = lean_where(bases, T2M, GM, N)
        plan.bind_mform(*ptrs[3:])
        launch_and_check(dev, b, plan, ptrs, "acm_tile2 byte-plane", where=where)
        launch_and_check(dev, b, plan, ptrs, "acm_tile2 byte-plane U16BE", fmt=capi.FMT_U16BE, where=where)
        plan.bind_mform(None, None)
        launch_and_check(dev, b, plan, ptrs, "acm_tile2 int16", where=lean_where(bases, T2, G2, units))
    finally:
        release(dev, plans, ptrs)


@pytest.mark.parametrize("level", [6, 7, 8, 9])
def test_packed_form_long_runs(dev, level):
    """acm_tile2p on the packed form (levels 6-9, default flags), runs of >= RUN_MIN tiles, S16LE and U16BE"""
    Lb = L()
    T2, G2 = Lb.acmk_tile2p_rows(level), Lb.acmk_tile2_grid(level, cus())      # (acm_tile2p has acm_tile2's tile geometry)
    assert T2 > 0 and G2 > 0 and T2 == Lb.acmk_tile2_rows(level) == capi.packed_tile_rows(level)
    units = size_units([(G2, 1)])
    b = Batch(level, T2, units, 90000 + 1000 * level, 16)
    pk = capi.pack_streams(b.ar.idx, b.descs, threads=THREADS)
    for k, h in enumerate(b.h1):
        if h:
            pk.streams[k].ntiles = 0
    bases, N = lean_layout(b, T2, T2)
    assert N == units and sum(s.ntiles for s in pk.streams) == N
    plans, ptrs = [], []
    try:
        ptrs = b.upload(dev) + list(pk.upload(dev))
        plan = capi.Plan(dev, b.descs, b.ar.patches, packed=pk.streams)
        plans.append(plan)
        assert plan.stats().packed_tiles == N
        plan.bind_packed(*ptrs[3:])
        where = lean_where(bases, T2, G2, N)
        launch_and_check(dev, b, plan, ptrs, "acm_tile2p", where=where)
        launch_and_check(dev, b, plan, ptrs, "acm_tile2p U16BE", fmt=capi.FMT_U16BE, where=where)
    finally:
        release(dev, plans, ptrs)


@pytest.mark.parametrize("level", [5, 6])
def test_fused_tile_long_runs(dev, level):
    """acm_fused_tile at levels 5 and 6: default flags (halo tiles: too few for the lean kernel at level 6), forced halo, and forced carry
    with runs of >= RUN_MIN tiles, S16LE and U16BE"""
    Lb = L()
    TC, G1 = Lb.acmk_fused_tile_rows(level, 0), Lb.acmk_fused_grid(level, 0, cus())
    assert TC > 2 and G1 > 0 and Lb.acmk_fused_has_carry(level, 0)
    unit = Lb.acmk_tile2_rows(level) or TC
    b = Batch(level, unit, -(-RUN_MIN * G1 * TC * 11 // (10 * unit)), 95000 + 1000 * level, 16)
    cnt = [fused_counts(b, k) for k in range(len(b.descs))]
    keep = fit([c[1] for c in cnt], G1)
    descs, patches = subset(b, keep)
    halo, carry, ex = (sum(c[j] for c in cnt[:keep]) for j in range(3))
    G2 = Lb.acmk_tile2_grid(level, cus())
    assert G2 == 0 or sum(b.whole_rows(k) // unit for k in range(keep) if not b.h1[k]) < 8 * G2      # (below the lean kernel's threshold)
    plans, ptrs = [], []
    try:
        ptrs = b.upload(dev)
        for flags, ntab in ((capi.PLAN_AUTO, halo), (capi.PLAN_FORCE_HALO, halo), (capi.PLAN_FORCE_CARRY, carry)):
            p = capi.Plan(dev, descs, patches, flags=flags)
            plans.append(p)
            st = p.stats()
            assert st.tiles == ntab + ex and st.stagewise_streams == 0, (flags, st.tiles, ntab, ex)
            where = None
            if flags == capi.PLAN_FORCE_CARRY:
                where = lean_where(table_layout([None if b.h1[k] else cnt[k][1] for k in range(keep)]), TC, G1, carry)
            launch_and_check(dev, b, p, ptrs, "acm_fused_tile, flags 0x%x" % flags, descs=descs, where=where)
            if flags != capi.PLAN_FORCE_HALO:
                launch_and_check(dev, b, p, ptrs, "acm_fused_tile, flags 0x%x, U16BE" % flags, descs=descs, fmt=capi.FMT_U16BE, where=where)
    finally:
        release(dev, plans, ptrs)


@pytest.mark.parametrize("level", [13, 14, 15])
def test_prefix_plane_long_runs(dev, level):
    """levels 13-15 on the prefix sweep + plane kernel (at 13 / 14 a batch below the lean kernel's threshold), many streams: halo tiles
    and carry runs of >= RUN_MIN tiles, S16LE and U16BE"""
    Lb = L()
    TP, GP = Lb.acmk_plane_tile_rows(), Lb.acmk_plane_grid(cus())
    assert TP > 2 and GP > 0
    unit = max(1, (TP << 12) >> level)                  # rows of this level in one carry tile of the plane (level-12 rows of 4096 samples)
    b = Batch(level, unit, -(-RUN_MIN * GP * 11 // 10), 97000 + 1000 * level, 2)
    emit12 = [(d.n_emit + 4095) >> 12 for d in b.descs]
    keep = fit([-(-e // TP) for e in emit12], GP)
    descs, patches = subset(b, keep)
    halo, carry = sum(-(-e // (TP - 2)) for e in emit12[:keep]), sum(-(-e // TP) for e in emit12[:keep])
    T2 = Lb.acmk_tile2_rows(level)
    if T2:
        assert sum(b.whole_rows(k) // T2 for k in range(keep) if not b.h1[k]) < 8 * Lb.acmk_tile2_grid(level, cus())
    carry_where = lean_where(table_layout([-(-e // TP) for e in emit12[:keep]]), TP, GP, carry)
    plans, ptrs = [], []
    try:
        ptrs = b.upload(dev)
        for flags, ntab in ((capi.PLAN_FORCE_HALO, halo), (capi.PLAN_FORCE_CARRY, carry)):
            p = capi.Plan(dev, descs, patches, flags=flags)
            plans.append(p)
            st = p.stats()
            assert st.tiles == ntab and st.mform_tiles == 0, (flags, st.tiles, ntab)
            where = (lambda k, row: carry_where(k, (row << level) >> 12)) if flags == capi.PLAN_FORCE_CARRY else None
            launch_and_check(dev, b, p, ptrs, "prefix + plane, flags 0x%x" % flags, descs=descs, where=where)
            launch_and_check(dev, b, p, ptrs, "prefix + plane, flags 0x%x, U16BE" % flags, descs=descs, fmt=capi.FMT_U16BE, where=where)
    finally:
        release(dev, plans, ptrs)
