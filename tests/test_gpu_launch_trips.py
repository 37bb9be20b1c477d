"""The launchers' second trips: what a launcher does with work that exceeds one grid.

Several launchers walk a list in slices (gridDim.y holds 65 535 streams or jobs: `d_list + at`, `d_jobs + at`), and several cap their
grid and let the kernel stride over the rest (`q += gridDim.x * SL_THREADS`, `work += gridDim.x`).  At the built-in limits
(include/acm_launch_caps.h) a second slice or a second trip takes 65 536 streams, 32 M samples of one level 0-4 stream or a million
dense work items, so nothing else in the suite walks these paths twice.  Here the handle's launch caps (acmhip_device_set_launch_caps,
tests only, lowers a limit and changes no result) put a handful of streams, jobs and rows through them, and three calls at real size
hold the built-in numbers themselves.

Every call goes into poisoned memory with guards, with the handle's fill mode on (helpers), and is compared bit for bit with what the
suite's own case lists and checkers expect: the oracle's decode for the synthesis kernels and the parser, the models of
tests/dense_*.py for the dense kernels.  No tolerance anywhere.

What the capped dense runs reach, and what they cannot show: with the grid capped at 1, 2 or 3 a workgroup works off many items one
behind the other, so the barriers that exist only for a second item of a workgroup - in front of filtered_sub_row in
acm_dense_resample / acm_dense_speed (the tap table and the planes in LDS are overwritten), behind the sum in acm_dense_energy
(part[]) - and the branch that is uniform within a workgroup but changes between its items are executed, deterministically.  A
MISSING barrier is a race: these tests fail on it only when the race happens to lose.
"""
import numpy as np
import pytest

import arena_contract as AC
import dense_crops as DC
import dense_mix as DM
import dense_overlay as DO
import dense_resample as DR
import dense_speed as DS
import helpers  # noqa: F401  (the fill mode of the handle, as in every module of GPU tests)
import test_gpu_arena_contract as T_CONTRACT
import test_gpu_dense_crops as T_CROPS
import test_gpu_dense_mix as T_MIX
import test_gpu_dense_overlay as T_OVERLAY
import test_gpu_dense_resample as T_RESAMPLE
import test_gpu_dense_speed as T_SPEED
import test_gpu_windows as T_WINDOWS
from helpers import fmt_args, make_stream, oracle_pcm
from libacm_amd import capi

pytestmark = pytest.mark.gpu

F32 = "f32"
SMALL_TRIP = 256 * 32                   # samples one workgroup of the level 0-4 register kernel writes per trip (SL_THREADS * SL_K)


# ================================================================================================ synthesis lists

_oracle = {}


def want_of(key, data, fmt):
    """the oracle's whole decode of a file in format fmt (uint16), or as float32 bits: computed once per file and format"""
    if (key, fmt) not in _oracle:
        if fmt == F32:
            _oracle[key, fmt] = AC.f32_bits(want_of(key, data, capi.FMT_S16LE))
        else:
            _oracle[key, fmt] = oracle_pcm(data, 0, *fmt_args(fmt))[0]
        _oracle[key, fmt].setflags(write=False)
    return _oracle[key, fmt]


_batch = None


def list_batch():
    """(files, staged, windows): the batch of test_gpu_parity.py::test_mixed_batch (levels 0, 3, 5, 7, 8, 9, 11, 12, 13), twenty more
    streams of levels 1, 2, 4, 14 and 15, and seven streams of levels 0-4 that one workgroup of the register kernel needs more than
    three trips for: a window from row 5 on of 3 * 8192 + 1013 samples (no multiple of 32: the last trip is ragged, and so is its
    last thread)"""
    global _batch
    if _batch is None:
        files = []
        for i in range(40):
            lv = [0, 3, 5, 7, 8, 9, 11, 12, 13][i % 9]
            rows = [1, 2, 16, 17, 33][i % 5] if lv < 13 else 2
            files.append(make_stream(500 + i, lv, rows, 1 + (i * 7) % 9, channels=1 + i % 2, cut=i % 4))
        for i in range(40, 60):
            lv = [1, 2, 4, 14, 15][i % 5]
            rows = [1, 2, 16, 17, 33][(i // 5) % 5] if lv < 13 else 2
            files.append(make_stream(500 + i, lv, rows, 1 + (i * 7) % 9, channels=1 + i % 2, cut=i % 4))
        windows = [None] * len(files)
        n_emit = 3 * SMALL_TRIP + 1013
        for j, lv in enumerate((0, 0, 1, 2, 3, 3, 4)):
            rows, cols = 997, 1 << lv
            nb = -(-(n_emit + 5 * cols) // (rows * cols)) + 1
            files.append(make_stream(560 + j, lv, rows, nb, cut=j))
            windows.append((5, n_emit))
        staged = [capi.stage_file(f) for f in files]
        windows = [w if w is not None else (0, s.words) for w, s in zip(windows, staged)]
        assert n_emit % 32 and n_emit > 3 * SMALL_TRIP
        _batch = (files, staged, windows)
    return _batch


def launch_arena(dev, ar, flags, fmt):
    """one plan over the arena's descriptors, launched into a poisoned PCM arena -> (the whole arena as written: uint16, or the bits of
    the floats; the plan's stats)"""
    f32 = fmt == F32
    unit, dt, byte = (4, np.uint32, 0xFF) if f32 else (2, np.uint16, 0xA5)
    d_idx, d_hdr, d_pcm = dev.malloc(ar.idx.nbytes), dev.malloc(ar.hdr.nbytes), dev.malloc(ar.pcm_words * unit)
    plan = None
    try:
        dev.memset(d_pcm, byte, ar.pcm_words * unit)
        dev.upload(d_idx, ar.idx)
        dev.upload(d_hdr, ar.hdr)
        plan = capi.Plan(dev, ar.descs, ar.patches, flags)
        if f32:
            plan.launch_f32(d_idx, d_hdr, d_pcm)
        else:
            plan.launch(d_idx, d_hdr, d_pcm, fmt)
        out = np.zeros(ar.pcm_words, dtype=dt)
        dev.download(out, d_pcm)
        return out, plan.stats()
    finally:
        if plan is not None:
            plan.destroy()
        for p in (d_idx, d_hdr, d_pcm):
            dev.free(p)


def poison_of(fmt):
    return np.uint32(0xFFFFFFFF) if fmt == F32 else np.uint16(0xA5A5)


@pytest.mark.parametrize("flags", [capi.PLAN_AUTO, capi.PLAN_STAGEWISE], ids=["auto", "stagewise"])
@pytest.mark.parametrize("list_slice", [1, 3])
def test_stream_lists_in_slices(dev, list_slice, flags):
    """acmk_launch_small (and its float32 twin), acmk_launch_unpack / stage / emit and acmk_launch_prefix with their lists cut into
    slices of 1 (`at` takes every value) and of 3 (a short last slice), the register kernel on ONE workgroup per stream: every stream
    is the oracle's, and no word between the streams' slots is written"""
    files, staged, windows = list_batch()
    ar = capi.Arena(staged, windows)
    by_level = {}
    for s in staged:
        by_level[s.info.level] = by_level.get(s.info.level, 0) + 1
    # the lists that are sliced: one per level (auto: the register kernel's and the prefix kernels'; stage-wise: every level's, and the
    # unpack launch's list of all streams) - longer than a slice, and some of them no multiple of it
    assert set(range(5)) | {13, 14, 15} <= set(by_level) and all(n > 3 for n in by_level.values())
    assert any(by_level[lv] % 3 for lv in range(5)) and any(by_level[lv] % 3 for lv in (13, 14, 15)) and len(staged) % 3
    # the register kernel on one workgroup: at least three whole trips and a ragged one for the long windows
    assert sum(1 for (rb, n), s in zip(windows, staged) if s.info.level <= 4 and rb > 0 and n > 3 * SMALL_TRIP and n % 32) >= 5
    inside = np.zeros(ar.pcm_words, dtype=bool)
    for (_, _, po, _, ne) in ar.layout:
        inside[po:po + ne] = True
    with dev.launch_caps(list_slice=list_slice, small_grid_x=1):
        for fmt in (capi.FMT_S16LE, capi.FMT_U16BE, F32):
            out, st = launch_arena(dev, ar, flags, fmt)
            if flags == capi.PLAN_AUTO:
                assert st.stagewise_streams == 0 and st.fused_streams == len(staged)     # the small and prefix lists are the ones sliced
            else:
                assert st.stagewise_streams == len(staged)
            for k, (f, s, (rb, ne), (_, _, po, _, _)) in enumerate(zip(files, staged, windows, ar.layout)):
                want = want_of(k, f, fmt)[rb << s.info.level:(rb << s.info.level) + ne]
                assert want.size == ne
                bad = np.nonzero(out[po:po + ne] != want)[0]
                assert bad.size == 0, "stream %d (level %d, rows %d, from row %d), format %s: %d of %d samples differ, the first at %d" % (
                    k, s.info.level, s.info.rows, rb, fmt, bad.size, ne, bad[0])
            assert (out[~inside] == poison_of(fmt)).all(), "format %s: a word between the streams' slots was written" % (fmt,)


CONTRACT_LEVELS = [0, 1, 2, 3, 4, 13, 14, 15]


@pytest.mark.parametrize("name", ["halo", "stagewise"])
@pytest.mark.parametrize("level", CONTRACT_LEVELS)
def test_sliced_lists_keep_the_arena_contract(dev, level, name):
    """test_gpu_arena_contract.py::test_plan_keeps_the_contract once more with the lists in slices of 3 and the register kernel on one
    workgroup per stream: 8-word offsets, ragged counts, windows - every slot the oracle's slice, no word written outside it.  "halo":
    the register kernel (levels 0-4; streams with H1 patches on the stage-wise kernels) and the prefix kernels (13-15)"""
    n = len(AC.contract(level).descs)
    assert n > 3
    with dev.launch_caps(list_slice=3, small_grid_x=1):
        T_CONTRACT.test_plan_keeps_the_contract(dev, level, name)


def test_65540_descriptors_cross_the_list_slice(dev):
    """The built-in slice itself: 65 540 descriptors over four staged level-2 streams, replicated as in
    test_gpu_parity.py::test_many_short_streams_stress_shape with distinct pcm_off and ragged n_emit - five more than gridDim.y holds,
    so acmk_launch_small (one plan) and acmk_launch_unpack, acmk_launch_stage and acmk_launch_emit (ACMHIP_PLAN_STAGEWISE) each launch a
    second slice of five streams from d_list + 65535.  int16 and float32.  The four streams are checked against the oracle at every
    replica (every block of four slots equals the first, the first is the oracle's), and the words between the slots keep their poison.
    The prefix kernels (levels 13-15) stay with the capped tests: 65 536 level-13 streams would need gigabytes of planes."""
    reps, pitch = 16385, 64
    files = [make_stream(8800 + k, 2, 5, 3, cut=k) for k in range(4)]
    staged = [capi.stage_file(f) for f in files]
    src = capi.Arena(staged)
    n_emit = [s.words - d for s, d in zip(staged, (0, 18, 3, 41))]
    assert all(0 < n < pitch for n in n_emit) and len({n % 4 for n in n_emit}) > 2
    descs = []
    for r in range(reps):
        for k, d in enumerate(src.descs):
            descs.append(capi.StreamDesc(idx_off=d.idx_off, hdr_off=d.hdr_off, pcm_off=len(descs) * pitch, n_emit=n_emit[k], level=d.level,
                                         rows=d.rows, nrows=d.nrows, row_begin=0))
    n = len(descs)
    assert n == 65540 > capi.LAUNCH_CAPS_BUILTIN["list_slice"]
    d_idx, d_hdr, d_pcm = dev.malloc(src.idx.nbytes), dev.malloc(src.hdr.nbytes), dev.malloc(n * pitch * 4)
    try:
        dev.upload(d_idx, src.idx)
        dev.upload(d_hdr, src.hdr)
        for flags in (capi.PLAN_AUTO, capi.PLAN_STAGEWISE):
            plan = capi.Plan(dev, descs, None, flags)
            try:
                st = plan.stats()
                assert (st.stagewise_streams, st.fused_streams) == ((n, 0) if flags == capi.PLAN_STAGEWISE else (0, n))
                for fmt in (capi.FMT_S16LE, F32):
                    f32 = fmt == F32
                    dev.memset(d_pcm, 0xFF if f32 else 0xA5, n * pitch * (4 if f32 else 2))
                    if f32:
                        plan.launch_f32(d_idx, d_hdr, d_pcm)
                    else:
                        plan.launch(d_idx, d_hdr, d_pcm, fmt)
                    out = np.zeros(n * pitch, dtype=np.uint32 if f32 else np.uint16)
                    dev.download(out, d_pcm)
                    blocks = out.reshape(reps, 4 * pitch)
                    first = blocks[0].reshape(4, pitch)
                    for k in range(4):
                        assert np.array_equal(first[k, :n_emit[k]], want_of(("65540", k), files[k], fmt)[:n_emit[k]]), (flags, fmt, k)
                        assert (first[k, n_emit[k]:] == poison_of(fmt)).all(), (flags, fmt, k)
                    differ = np.nonzero((blocks != blocks[0]).any(axis=1))[0]
                    assert differ.size == 0, "plan flags %d, format %s: %d of %d replicas differ from the first, the first of them replica %d" % (
                        flags, fmt, differ.size, reps, differ[0])
            finally:
                plan.destroy()
    finally:
        for p in (d_idx, d_hdr, d_pcm):
            dev.free(p)


# ================================================================================================ the device parser

_parser_files = None


def parser_files():
    """the files of test_gpu_parity.py::test_device_parser_every_filler with 120 of its 300 synthetic streams: every filler code, a WAVC
    prefix, ragged rows, six hazard-H1 streams and a truncated file (both flagged by the device: the host reader takes them)"""
    global _parser_files
    if _parser_files is None:
        from helpers import golden, golden_file
        g = golden()
        files = [golden_file(c["file"]) for fam in ("F1_matrix", "F2_codes", "F6_headers") for c in g[fam] if c["open"] == 0]
        files += [golden_file("f5_wavc"), golden_file("f5_plain")]
        files += [make_stream(5200 + i, [5, 6, 7, 8, 3, 10][i % 6], [16, 7, 1, 33, 512, 600][i % 6], 1 + i % 4, channels=1 + i % 2, cut=i % 5)
                  for i in range(120)]
        h1 = len(files)
        files += [make_stream(5900 + i, 6, 8, 3, prime_table=1, allow_out_of_range=1) for i in range(6)]
        whole = make_stream(5990, 7, 16, 10)
        files.append(whole[:len(whole) * 2 // 3])
        _parser_files = (files, list(range(h1, len(files))))
    return _parser_files


_parser_ref = {}


def parser_reference(dev, ranges, byteplane):
    """(the host parse, the uncapped device parse's timing) of the parser files: once per way of staging"""
    if (ranges, byteplane) not in _parser_ref:
        files, _ = parser_files()
        if "host" not in _parser_ref:
            _parser_ref["host"] = capi.batch_decode(dev, files, threads=4, parse=capi.PARSE_HOST)[0]
        _, tm = capi.batch_decode(dev, files, threads=4, parse=capi.PARSE_DEVICE, byteplane=byteplane)
        _parser_ref[ranges, byteplane] = (_parser_ref["host"], int(tm.device_parsed), int(tm.host_parsed))
    return _parser_ref[ranges, byteplane]


@pytest.mark.parametrize("byteplane", [False, True], ids=["int16", "byteplane"])
@pytest.mark.parametrize("ranges", [1, 3])
@pytest.mark.parametrize("parse_slice", [1, 5])
def test_column_kernel_in_slices(dev, parse_slice, ranges, byteplane, monkeypatch):
    """launch_columns (acm_parse.hip) with its job table cut into slices of 1 and of 5 (`d_jobs + at`, `d_res + at`, `d_flags + at`)
    and ONE workgroup per job striding over the job's columns: the PCM and the statuses are the host parse's, a sample of them the
    oracle's, as many streams stay on the device as without caps, and the streams the device flags - H1, a truncated file - are still
    the ones the host reader takes"""
    monkeypatch.setattr(capi, "BATCH_EXTRA", capi.batch_ranges(ranges))
    files, flagged = parser_files()
    host, dev_parsed, host_parsed = parser_reference(dev, ranges, byteplane)
    assert dev_parsed > 100 and dev_parsed % 5 and host_parsed >= len(flagged)
    with dev.launch_caps(parse_slice=parse_slice, parse_grid_x=1):
        got, tm = capi.batch_decode(dev, files, threads=4, parse=capi.PARSE_DEVICE, byteplane=byteplane)
    assert (tm.device_parsed, tm.host_parsed) == (dev_parsed, host_parsed)
    for k, ((hs, hp), (ds, dp)) in enumerate(zip(host, got)):
        assert hs == ds and np.array_equal(hp, dp), k
    for k in list(range(0, len(files), 7)) + flagged:
        want, status = oracle_pcm(files[k])
        assert np.array_equal(got[k][1], want) and (got[k][0] == 0 or status < 0), k


@pytest.mark.parametrize("parse_slice", [1, 5])
def test_window_matrix_with_the_column_kernel_in_slices(dev, parse_slice):
    """test_gpu_windows.py::test_window_matrix at level 7 - acm_parse_scan_blocks, then the column kernel over a job per window - with
    the same caps"""
    with dev.launch_caps(parse_slice=parse_slice, parse_grid_x=1):
        T_WINDOWS.test_window_matrix(dev, 7)


# ================================================================================================ the dense kernels

def dense_units(frames, channels, planar):
    """(units per sub-row, sub-rows per row) of a dense launch, a model of its own of dense_geo() in libacm_amd/csrc/acm_dense_geo.h, which
    every dense launcher asks - a unit is 256 lanes of 8 samples, and the samples behind the last whole vector go with the last unit"""
    subs = 2 if planar and channels == 2 else 1
    sub_len = frames if subs == 2 else frames * channels
    return max(1, (sub_len // 8 + 255) // 256), subs


def trips_of(nrows, per_row, grid, kind):
    """the items of a launch of nrows * per_row work items on `grid` workgroups, as the kernels' loops hand them out (work = blockIdx.x,
    += gridDim.x; row = work / per_row) -> (items of workgroup 0, the set of (kind of an item, kind of the same workgroup's next one))"""
    nwork = nrows * per_row
    pairs = set()
    for g in range(min(grid, nwork)):
        rows = [w // per_row for w in range(g, nwork, grid)]
        pairs |= {(kind(a), kind(b)) for a, b in zip(rows, rows[1:])}
    return len(range(0, nwork, grid)), pairs


def resample_row_is_filtered(case, k):
    """acm_dense_layout.cpp: a row is filtered (L != 0) when its window has a ratio and delivers samples"""
    return bool(case.filtered(k) and case.expect(k)[0] > 0)


def speed_row_is_filtered(case, k, mix, rate):
    """... with either filter (a DS.Case, or a DO.Case whose windows are gathered with ACM_DENSE_MIX at DO.RATE)"""
    f = case.windows[k][0]
    if f >= len(DR.files()) or DS.turned_away(f, case.channels, mix, rate, case.speeds[k]):
        return False
    return DS.filter_of(f, rate, case.speeds[k])[0].kind in ("exact", "wide") and case.expect(k)[0] > 0


FILTERED, PLAIN = True, False
ALL_PAIRS = {(FILTERED, FILTERED), (FILTERED, PLAIN), (PLAIN, FILTERED)}


def dense_calls(family, f32):
    """the calls of a family's expected-rows matrix with the device parser: (run the call and check it, nrows, (units, subs), kind of row
    k) per call - and for an overlay call the launches behind the gather as further entries that run nothing"""
    dev_parse = capi.PARSE_DEVICE
    if family == "crops":
        for case in DC.cases():
            for planar in (False, True):
                yield (lambda d, c=case, p=planar: T_CROPS.test_expected_rows(d, c, f32, p, dev_parse), len(case.windows),
                       dense_units(case.frames, case.channels, planar), lambda k: PLAIN)
    elif family == "mix":
        for case in DM.cases():
            for planar in (False, True):
                yield (lambda d, c=case, p=planar: T_MIX.test_expected_rows(d, c, f32, p, dev_parse), len(case.windows),
                       dense_units(case.frames, case.channels, planar), lambda k: PLAIN)
    elif family == "resample":
        for case in DR.cases():
            for planar in (False, True):
                yield (lambda d, c=case, p=planar: T_RESAMPLE.test_expected_rows(d, c, f32, p, dev_parse), len(case.windows),
                       dense_units(case.frames, case.channels, planar), lambda k, c=case: resample_row_is_filtered(c, k))
    elif family == "speed":
        for case in DS.cases():
            for planar in (False, True):
                yield (lambda d, c=case, p=planar: T_SPEED.test_expected_rows(d, c, f32, p, dev_parse), len(case.windows),
                       dense_units(case.frames, case.channels, planar),
                       lambda k, c=case: speed_row_is_filtered(c, k, c.mix, c.rate))
    else:
        for case in DO.cases():
            # the gather that writes the source rows (acm_dense_speed: the windows have speeds), ...
            yield (lambda d, c=case: T_OVERLAY.test_expected_rows(d, c, f32, dev_parse), len(case.windows),
                   dense_units(case.frames, case.channels, case.planar),
                   lambda k, c=case: speed_row_is_filtered(c, k, True, DO.RATE))
            # ... acm_dense_energy over the rows whose energy a record asks for (units of 2048 samples of the whole row), ...
            marked = {x for rec in case.records if rec[1] is not None and rec[3] for x in rec[:2]}
            yield (None, len(marked), (-(-case.row // 2048), 1), lambda k: PLAIN)
            # ... and acm_dense_overlay over the output rows
            yield (None, len(case.records), dense_units(case.row, 1, False), lambda k: PLAIN)


FAMILIES = ["crops", "mix", "resample", "speed", "overlay"]


def coverage_of(family, f32, grid):
    """what a capped run of the family gives its workgroups, from the case lists and the geometry alone: every launch hands workgroup 0
    at least two items, and in EVERY call of the families that filter (the overlay family: in its gathers taken together) a workgroup
    goes from a filtered item to a filtered one, from a filtered one to a plain one and back"""
    pairs = set()
    for call, nrows, (units, subs), kind in dense_calls(family, f32):
        mine, p = trips_of(nrows, units * subs, grid, kind)
        assert mine >= 2, (family, grid, nrows, units, subs)
        assert family not in ("resample", "speed") or ALL_PAIRS <= p, (family, grid, nrows, units, subs, p)
        pairs |= p
    assert family not in ("resample", "speed", "overlay") or ALL_PAIRS <= pairs, (family, grid, pairs)
    return pairs


@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("grid", [1, 2, 3])
@pytest.mark.parametrize("family", FAMILIES)
def test_dense_kernels_on_a_capped_grid(dev, family, grid, f32):
    """the family's expected-rows matrix (its own case list, its own checker, the device parser) with every dense launch on 1, 2 or 3
    workgroups.  1: one workgroup works off every item in order - the resample cases alternate plain and filtered rows, so neighbouring
    items change kind.  2: on rows of one unit a workgroup gets every second row - filtered behind filtered, a new table over the old
    one.  3: coprime to the two sub-rows of planar stereo and to the two units of the 2100-frame rows"""
    coverage_of(family, f32, grid)
    with dev.launch_caps(dense_grid=grid):
        for call, _, _, _ in dense_calls(family, f32):
            if call is not None:
                call(dev)


def test_2_to_the_20_plus_7_overlay_rows_cross_the_dense_grid(dev):
    """The built-in dense grid itself: one overlay call with 2^20 + 7 output rows of 8 mono frames over the eleven source windows of
    a dense_overlay case.  acm_dense_overlay has one work item per row here, so the workgroups 0..6 take a second trip (work +=
    gridDim.x = 2^20); acm_dense_gains, which has a thread per row and no loop, crosses the same number in its row index.  The records:
    the case's own (a, b, vol, snr, gain) tuples in a seeded order, and one that occurs only in the last seven rows.  Expected rows,
    gains and energies are made once per distinct record by tests/dense_overlay.py's model and compared through the index array; a row
    nobody wrote would keep the buffer's poison (0xC7C7, which no expected row consists of)"""
    case = DO.build_case(1, 8, False)
    sources = case.sources()
    only_late = (DO.WIDE, DO.SPEECH, 3333, DO.SNR_5, 0)
    distinct = list(dict.fromkeys(case.records)) + [only_late]
    assert len(distinct) >= 24 and only_late not in case.records
    made = [DO.row_of(sources, rec) for rec in distinct]
    want_rows = np.stack([m[0] for m in made]).view(np.uint16)
    want_gain = np.array([m[1] for m in made], dtype=np.uint64)
    n = (1 << 20) + 7
    assert n > capi.LAUNCH_CAPS_BUILTIN["dense_grid"]
    rng = np.random.default_rng(1 << 20)
    which = rng.integers(0, len(distinct) - 1, n)
    which[n - 3] = len(distinct) - 1
    assert (which[:n - 7] != len(distinct) - 1).all()
    table = np.zeros(n, dtype=capi.OVERLAY_ROW_DT)
    recs = np.array([(a, capi.OVERLAY_NONE if b is None else b, vol, snr, g) for a, b, vol, snr, g in distinct], dtype=np.uint32)
    for col, name in enumerate(("a", "b", "vol", "snr", "gain")):
        table[name] = recs[which, col]
    files, index = T_OVERLAY.data_and_index()
    got, (st, words, offsets, res, tm) = T_OVERLAY.poisoned(dev, n, case.row, False, 0, lambda d, nwords: capi.batch_decode_windows_overlay(
        dev, files, index, case.windows, table, d, nwords, case.frames, channels=1, planar=False, f32=False, parse=capi.PARSE_DEVICE, threads=4,
        mix=True, rate=DO.RATE, speeds=case.speeds, result_table=True))
    for k in range(len(case.windows)):
        assert (words[k], st[k]) == case.expect(k), (k, case.windows[k])
    poison = np.uint16(T_OVERLAY.POISON * 0x101)
    assert not (want_rows == poison).all(axis=1).any()
    bad = np.nonzero((got != want_rows[which]).any(axis=1))[0]
    assert bad.size == 0, "%d of %d rows differ, the first row %d (record %r), %d of them still poison" % (
        bad.size, n, bad[0], distinct[which[bad[0]]], int((got[bad] == poison).all(axis=1).sum()))
    for col, name in enumerate(("gain", "energy_a", "energy_b")):
        assert np.array_equal(res[name].astype(np.uint64), want_gain[which, col]), name
