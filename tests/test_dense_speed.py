"""Dense crop batches with a speed per window without a GPU: ACM_DENSE_SPEED in the device-free half of acm_batch_decode_windows_dense
(libacm_amd/csrc/acm_dense_layout.cpp, acm_resample_layout.cpp), the case list of tests/dense_speed.py, and the code the compiler makes
of the kernel (libacm_amd/csrc/acm_dense_speed.hip).

  * acm_dense_speed_taps() against the contract: the wide tables equal the numpy design up to how libm and numpy round a double, every
    phase sums to 16384 and cannot overflow 32 bits; the classification of the contract's examples.
  * acmk_dense_speed_layout_visit(): the "speed" and "speed_tables" tables of every case, the soft refusals, every refusal of a whole
    call, the 17th table; and that without flag 32 nothing is read of a window's speed.
  * the definition itself: the wide filter against the exact one where both exist.
  * what the case list reaches, asserted here so that the GPU tests over the same list cannot pass vacuously.
  * the device-free half under AddressSanitizer and UBSan, as a program of its own (tests/native/speed_layout.cpp).
  * acm_dense_speed.hip compiled to gfx950 assembly: no scratch, 63 KB of LDS, 16-byte global loads and stores."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_resample as DR
import dense_speed as DS
import test_dense_crops as TD
import test_dense_resample as TR
import test_window_layout as WL
from libacm_amd import _build, batch, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS, SP = capi.DENSE_RESAMPLE, capi.DENSE_SPEED
ALL_ONES = 2 ** 64 - 1
KIND = {"none": 0, "exact": 1, "wide": 2, "bad": ALL_ONES}


def ratio_of_cutoff(c):
    """(rate_in, rate_out, speed) of a wide row with cutoff c: 64 L / M = (c + 0.5) * 1.001 below 64, any odd upsampling for 64"""
    return (16000, 22051, None) if c == 64 else (64000, c * 1000 + 500, (1000, 1001))


# ---------------------------------------------------------------------------------------------------------------- the tables

@pytest.mark.parametrize("c", [8, 9, 23, 46, 63, 64])
def test_wide_tables_are_the_contracts(c):
    ri, ro, speed = ratio_of_cutoff(c)
    flt = DS.Filter(ri, ro, speed)
    assert flt.kind == "wide" and flt.c == c
    info, q = capi.dense_speed_taps(ri, ro, speed or (1, 1))
    K, Wd, P, b = DS.wide_shape(c)
    assert (capi.SPEED_KINDS[info.kind], info.L, info.M, info.K, info.Wd, info.P, info.c, info.phases, info.step) == \
        ("wide", flt.L, flt.M, K, Wd, P, c, P + 1, (flt.M << 32) // flt.L)
    assert (P + 1) * K <= 16384 < (2 * P + 1) * K and P == 1 << b and q.shape == (P + 1, K) and q.dtype == np.int16
    q = q.astype(np.int64)
    assert (q.sum(axis=1) == 16384).all()
    assert np.abs(q).sum(axis=1).max() < 65536
    # the numpy design: libm and numpy may round a double apart, by one; the tap that makes up the sum follows the others
    want = DS.design_wide(c)
    off = np.abs(q - want)
    fix = want.argmax(axis=1)
    others = off.copy()
    others[np.arange(P + 1), fix] = 0
    assert others.max() <= 1
    assert (off[np.arange(P + 1), fix] <= 1 + (others != 0).sum(axis=1)).all()
    # the last phase is the first one a source frame on
    assert (q[P, 1:] == q[0, :-1]).all() or np.abs(q[P, 1:] - q[0, :-1]).max() <= 1


def test_table_shapes_of_the_contract():
    assert [DS.wide_shape(c)[::2] for c in (64, 63, 23, 8)] == [(16, 512), (18, 512), (46, 256), (128, 64)]
    for c in range(8, 65):
        K, Wd, P, b = DS.wide_shape(c)
        assert 16 <= K <= 128 and (P + 1) * K <= 16384 and 17 - b >= 0
        assert np.abs(DS.design_wide(c)).sum(axis=1).max() <= 33588


# ---------------------------------------------------------------------------------------------------------------- the classification

CLASSES = [((22050, 16000, (9, 10)), ("wide", 3200, 3969), dict(c=51, K=22, P=512)),
           ((22050, 16000, (11, 10)), ("wide", 3200, 4851), dict(c=42, K=26)),
           ((44100, 16000, (11, 10)), ("wide", 1600, 4851), dict(c=21, K=50, P=256)),
           ((22050, 22050, (9, 10)), ("exact", 10, 9), dict(K=16)),
           ((22051, 22050, None), ("wide", 22050, 22051), dict(c=63)),
           ((16000, 16000, (1001, 1000)), ("wide", 1000, 1001), dict(c=63)),
           ((22050, 2450, None), ("bad", 1, 9), {}),
           ((22050, 22050, (9, 1)), ("bad", 1, 9), {}),
           ((22050, 22050, (3, 3)), ("none", 1, 1), {}),
           ((16000, 22050, None), ("exact", 441, 320), dict(K=16)),
           ((22048, 2756, None), ("exact", 1, 8), dict(K=128)),
           ((16000, 2050, (999, 1000)), ("wide", 1025, 7992), dict(c=8, K=128, P=64)),
           ((8000, 4294967291, (65535, 65534)), ("bad", 4294967291 * 32767, 4000 * 65535), {})]


@pytest.mark.parametrize("args,want,more", CLASSES, ids=["%d_%d_at_%d_%d" % (a[0], a[1], *(a[2] or (1, 1))) for a, _, _ in CLASSES])
def test_classification(args, want, more):
    ri, ro, speed = args
    flt = DS.Filter(ri, ro, speed)
    assert (flt.kind, flt.L, flt.M) == want and all(getattr(flt, k) == v for k, v in more.items())
    if flt.kind == "bad":
        with pytest.raises(ValueError):
            capi.dense_speed_taps(ri, ro, speed or (1, 1))
        assert capi.dense_speed_frames(100, ri, ro, speed or (1, 1)) is None
        return
    info, q = capi.dense_speed_taps(ri, ro, speed or (1, 1))
    assert capi.SPEED_KINDS[info.kind] == flt.kind
    if flt.kind == "none":
        assert (info.L, info.M, info.K, info.Wd, info.phases) == (1, 1, 16, 8, 1) and q[0, 7] == 16384 and np.count_nonzero(q) == 1
    else:
        assert (info.L, info.M, info.K, info.Wd) == (flt.L, flt.M, flt.K, flt.Wd)
    if flt.kind == "exact":
        assert (info.P, info.c, info.step, info.phases) == (0, 0, 0, flt.L)
    for f in (0, 1, 999, 1000, 12345):
        assert capi.dense_speed_frames(f, ri, ro, speed or (1, 1)) == flt.n_out(f)
    assert batch.source_frames(2100, ri, ro, speed or (1, 1)) == flt.longest(2100)


def test_an_exact_table_is_a_function_of_l_and_m():
    """speed 9/10 at equal rates is the table of 10 : 9 whatever made that ratio - bit for bit what acm_dense_resample_taps hands out"""
    a = capi.dense_speed_taps(22050, 22050, (9, 10))[1]
    assert np.array_equal(a, capi.dense_resample_taps(9, 10)[4]) and np.array_equal(a, capi.dense_speed_taps(44100, 24500, (1, 2))[1])
    assert np.array_equal(capi.dense_speed_taps(16000, 22050)[1], capi.dense_resample_taps(16000, 22050)[4])
    # the two helpers of ACM_DENSE_RESAMPLE keep their answers: an odd rate is still none of theirs
    with pytest.raises(ValueError):
        capi.dense_resample_taps(22051, 22050)
    assert capi.dense_resampled_frames(100, 22051, 22050) is None and capi.dense_speed_frames(100, 22051, 22050) == 100


# ---------------------------------------------------------------------------------------------------------------- the layout

def _lib():
    L = capi.lib()
    L.acmk_dense_speed_layout_visit.argtypes = [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                WL.VISIT, C.c_void_p]
    return L


def call(items, wins, speeds, frames, channels, dense_flags=RS | SP, rate=DR.RATE, parse=capi.PARSE_HOST, final_words=None):
    """tests/test_dense_resample.py::call through the visitor that takes the windows' speeds: (num, den) pairs, None for 0, or a raw word"""
    n, nwin = len(items), len(wins)
    info = (capi.StageInfo * max(n, 1))()
    length, whole = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
    ok, end_status, blocks = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint32)
    marks = (C.c_void_p * max(n, 1))()
    for i, it in enumerate(items):
        f = it.info
        info[i] = capi.StageInfo(f.level, f.rows, f.cols, f.channels, f.channels, f.rate, f.total_values, 0, f.blocks, f.end_status, 0, f.header_bytes)
        length[i], whole[i], ok[i], end_status[i], blocks[i] = it.len, it.whole, it.ok, it.end_status, f.blocks
        marks[i] = it.marks.ctypes.data if it.marks is not None else None
    win3 = np.array([w[:3] for w in wins], dtype=np.uint64).reshape(-1)
    raw = np.array([0 if s is None else s if isinstance(s, int) else s[0] << 16 | s[1] for s in (speeds or [None] * nwin)], dtype=np.uint32)
    opts = capi.BatchOpts(0, capi.FMT_S16LE, 4, 0, parse, 0, TD.FAKE_PTR, nwin * frames * channels, None)
    dense = capi.DenseOpts(frames, channels, dense_flags, rate, 0)
    final = None if final_words is None else np.array(final_words, dtype=np.uint64)
    tables = {}

    def visit(_ctx, name, data, elem_bytes, count):
        assert name.decode() not in tables and elem_bytes % 8 == 0
        tables[name.decode()] = np.frombuffer(C.string_at(data, elem_bytes * count), dtype="<u8").reshape(count, elem_bytes // 8).copy()
    rc = _lib().acmk_dense_speed_layout_visit(info, length.ctypes.data, ok.ctypes.data, end_status.ctypes.data, whole.ctypes.data, marks,
                                              blocks.ctypes.data, n, win3.ctypes.data if nwin else None, raw.ctypes.data if speeds is not None else None,
                                              nwin, C.byref(opts), C.byref(dense), final.ctypes.data if final is not None else None, WL.VISIT(visit), None)
    tot = dict(zip(TD.TOTALS, tables["totals"].reshape(-1).astype(np.int64).tolist()))
    assert tot["rc"] == rc
    return rc, tables, tot


@pytest.fixture(scope="module")
def items():
    return [DR.layout_item(f) for f in DR.files()]


@pytest.mark.parametrize("case", DS.cases(), ids=lambda c: c.name)
def test_layout_tables(items, case):
    flags = RS | SP | (capi.DENSE_MIX if case.mix else 0)
    rc, got, tot = call(items, case.windows, case.speeds, case.frames, case.channels, dense_flags=flags, rate=case.rate, parse=capi.PARSE_DEVICE)
    assert rc == 0 and list(got) == TR.PLAIN_TABLES[:-1] + (["mix"] if case.mix else []) + ["speed", "speed_tables", "totals"]
    tabs, res, n = got["speed_tables"].tolist(), got["speed"].tolist(), len(case.windows)
    assert 2 <= len(tabs) <= 16 and res[n] == [2, 0, 0, 0, 0, 0, 0, 0]
    at, keys = 0, []
    for wide, c, L, M, K, Wd, phases, off in tabs:              # in the order of their first window, 16-byte lines apart
        assert off == at and off % 8 == 0 and phases * K <= 16384
        assert (K, Wd, phases) == ((DS.wide_shape(c)[0], DS.wide_shape(c)[1], DS.wide_shape(c)[2] + 1) if wide else (DS.Filter(M, L).K, DS.Filter(M, L).Wd, L))
        keys.append(c if wide else (L, M))
        at += -(-phases * K // 8) * 8
    assert len(set(keys)) == len(keys) and tot["table_bytes"] == 16 * n + 48 * n + 2 * at
    nblocks = 0
    for k in range(n):
        words, status, nb = case.expect(k)
        nblocks += nb
        assert tuple(TD.signed(got["report"])[k][:2]) == (status, words) and words == case.delivers(k), (case.name, k)
        flt = case.filter(k)
        kind, L, M, tid, frames_out, step, b, Wd = res[k]
        assert frames_out == case.frames_out(k) <= case.frames, (case.name, k)
        if flt is not None and flt.key is not None and words:
            assert (kind, L, M, Wd, keys[tid]) == (KIND[flt.kind], flt.L, flt.M, flt.Wd, flt.key), (case.name, k)
            assert (step, b) == ((flt.step, flt.b) if flt.kind == "wide" else (0, 0))
        else:
            away = flt is None and case.windows[k][0] < len(DR.files()) and (case.mix or DR.chans_of(case.windows[k][0], case.channels) == case.channels)
            assert (kind, L, M, tid, step) == ((ALL_ONES, 0, 0, ALL_ONES, 0) if away else (0, 1, 1, ALL_ONES, 0)), (case.name, k)
        assert int(got["rejected"][k][0]) == int(flt is None and case.windows[k][0] < len(DR.files()))
    assert tot["blocks_parsed"] == nblocks


def test_which_kernel_takes_the_launch(items):
    """what staging left decides: a wide row that got samples makes it acm_dense_speed (2), an exact one alone acm_dense_resample (1),
    neither the kernel of a call without the flags (0); and a call whose speeds make no row wide has the tables of the call without flag 32"""
    wins, speeds = [(2, 8, 40), (2, 3, 50), (0, 5, 30), (2, 0, 64)], [(9, 10), DS.NEAR_ONE, None, (4, 4)]
    rc, got, tot = call(items, wins, speeds, 64, 1)
    assert rc == 0 and [r[0] for r in got["speed"].tolist()] == [1, 2, 1, 0, 2] and tot["table_bytes"] == 4 * 64 + 2 * (160 + 513 * 16 + 32)
    rc, got, _ = call(items, wins, speeds, 64, 1, final_words=[40, 0, 30, 64])
    assert rc == 0 and [r[0] for r in got["speed"].tolist()] == [1, 0, 1, 0, 1]
    rc, got, _ = call(items, wins, speeds, 64, 1, final_words=[0, 0, 0, 64])
    assert rc == 0 and [r[0] for r in got["speed"].tolist()] == [0, 0, 0, 0, 0]
    # no wide table: 32 bytes a row behind the row table, as without the flag
    wins, speeds = [(0, 5, 30), (4, 16, 128), (2, 0, 64), (6, 2, 46)], [None, (1, 1), (7, 7), None]
    rc0, plain, tot0 = TR.call(items, wins, 64, 1)
    rc1, got, tot1 = call(items, wins, speeds, 64, 1)
    assert rc0 == rc1 == 0 and tot0 == tot1 and got["speed"][-1][0] == 1
    for name in TR.PLAIN_TABLES:
        assert plain[name].tobytes() == got[name].tobytes(), name
    assert [t[2:6] + t[7:] for t in got["speed_tables"].tolist()] == [t[1:] for t in plain["tables"].tolist()]
    assert [r[1:5] for r in got["speed"].tolist()[:-1]] == [r[:4] for r in plain["resample"].tolist()[:-1]]


def test_refusals_of_a_whole_call(items):
    wins, T = [(2, 8, 32), (4, 16, 128), (0, 4, 32)], 64
    sp = [(9, 10), None, (1001, 1000)]
    assert call(items, wins, sp, T, 1)[0] == 0
    for what, w, s, kw in (("the flag without ACM_DENSE_RESAMPLE", wins, sp, dict(dense_flags=SP)),
                           ("an unknown flag", wins, sp, dict(dense_flags=RS | SP | 64)),
                           ("no denominator", wins, [9 << 16, None, None], {}), ("no numerator", wins, [None, 10, None], {}),
                           ("one frame too long at 9/10", wins + [(2, 0, 58)], sp + [(9, 10)], {}),
                           ("one frame too long at 29999/30000", wins + [(2, 0, 64)], sp + [DS.NEAR_ONE], {}),
                           ("one frame too long at 22051 Hz", wins + [(8, 0, 65)], sp + [None], {}),
                           ("far too long", wins + [(8, 0, 1 << 62)], sp + [None], {}),
                           ("too long for a window that is turned away", wins + [(4, 0, 65)], sp + [(5, 1)], {}),
                           ("frames of 2^28", [], [], dict(frames=1 << 28))):
        rc, tables, tot = call(items, w, s, kw.pop("frames", T), 1, **kw)
        assert rc == capi.ERR_ARG and list(tables) == ["totals"], what
    for what, w, s in (("the longest window at 9/10", (2, 0, 57), (9, 10)), ("the longest at 29999/30000", (2, 0, 63), DS.NEAR_ONE),
                       ("the longest at 22051 Hz", (8, 0, 64), None), ("the longest at 11/10 from 44100 Hz", (4, 0, 140), (11, 10))):
        rc, tables, tot = call(items, wins + [w], sp + [s], T, 1)
        assert rc == 0 and int(tables["speed"][3][4]) == T, what
    assert call(items, [], [], (1 << 28) - 1, 1)[0] == 0
    # a ratio beyond an eighth is turned away softly, and nothing of it is parsed
    rc, alone, tot0 = call(items, wins, sp, T, 1)
    rc, got, tot = call(items, wins[:1] + [(4, 8, 64)] + wins[1:], sp[:1] + [(5, 1)] + sp[1:], T, 1)
    assert rc == 0 and tot["blocks_parsed"] == tot0["blocks_parsed"] > 0 and TD.signed(got["report"])[1][:2] == (capi.ERR_ARG, 0)
    assert got["speed"].tolist()[1] == [ALL_ONES, 0, 0, ALL_ONES, 0, 0, 0, 0] and [got["speed"].tolist()[k] for k in (0, 2, 3)] == alone["speed"].tolist()[:3]


def test_the_seventeenth_table(items):
    """exact (L, M) tables and wide c tables are counted together"""
    rates = [22050 * a // b for a, b in ((1, 2), (2, 1), (1, 3), (3, 1), (2, 3), (3, 2), (1, 5), (5, 1), (2, 5), (5, 2), (3, 5), (5, 3), (1, 6), (1, 7),
                                         (7, 1))]
    its = [TR.with_rate(items[2], r) for r in rates] + [items[2]]
    wins = [(k, 0, 8) for k in range(14)] + [(15, 0, 8), (15, 0, 8)]
    sp = [None] * 14 + [DS.NEAR_ONE, (1001, 1000)]
    rc, tables, tot = call(its, wins, sp, 64, 1)
    assert rc == 0 and tables["speed_tables"].shape == (16, 8) and [t[0] for t in tables["speed_tables"].tolist()] == [0] * 14 + [1, 1]
    assert call(its, wins * 3 + [(0, 0, 8)], sp * 3 + [DS.NEAR_ONE], 64, 1)[0] == 0              # c = 64 again
    assert call(its, wins + [(14, 0, 8)], sp + [None], 64, 1)[0] == capi.ERR_ARG                   # a 15th exact table
    assert call(its, wins + [(1, 0, 8)], sp + [(1001, 1000)], 64, 1)[0] == capi.ERR_ARG           # a third wide one: c = 31
    assert DS.Filter(44100, 22050, (1001, 1000)).key == 31


def test_without_the_flag_a_speed_is_not_read(items):
    """flag 32 off: the existing visitor's tables for tests/dense_resample.py's cases, and the same tables whatever `reserved` holds"""
    for case in DR.cases():
        flags = RS | (capi.DENSE_MIX if case.mix else 0)
        rc0, want, tot0 = TR.call(items, case.windows, case.frames, case.channels, dense_flags=flags)
        rc1, got, tot1 = call(items, case.windows, [0xFFFFFFFF, 9 << 16, 7] * (len(case.windows) // 3 + 1), case.frames, case.channels, dense_flags=flags)
        assert rc0 == rc1 == 0 and tot0 == tot1 and list(want) == list(got) and "tables" in want and "speed" not in want
        for name in want:
            assert want[name].tobytes() == got[name].tobytes(), (case.name, name)
        # ... which are what they were: the ratios of the three rates, the odd one turned away
        assert sorted(t[:5] for t in TD.signed(want["tables"])) == sorted((r,) + DR.ratio(r, DR.RATE) for r in (11025, 16000, 44100))
        assert all(r[4] == (1 if w[0] == 8 and (case.mix or case.channels == 1) else 0) for r, w in zip(want["resample"].tolist(), case.windows))


# ---------------------------------------------------------------------------------------------------------------- the definition

def test_wide_agrees_with_exact_where_both_exist():
    """16000 -> 22050 on 4000 frames of uniform full-scale noise: measured rms 1.93 and max 10 LSB; a wrong phase direction or a tap off
    by one gives thousands"""
    x = np.random.default_rng(1).integers(-32768, 32768, 4000)
    exact, q = DS.table(16000, 22050)
    assert exact.kind == "exact"
    wide = DS.Filter(16000, 22050)
    wide.kind, wide.c = "wide", 64
    wide.K, wide.Wd, wide.P, wide.b = DS.wide_shape(64)
    wide.step = (wide.M << 32) // wide.L
    library = capi.dense_speed_taps(16000, 22051)[1].astype(np.int64)       # every upsampling ratio shares the table of c = 64
    d = DS.wide_frames(x, wide, library).astype(np.int64) - DS.resample(x, exact, q)
    rms, top = float(np.sqrt((d ** 2).mean())), int(np.abs(d).max())
    print("wide against exact: rms %.2f LSB, max %d LSB" % (rms, top))
    assert d.size == 5513 and rms <= 4 and top <= 32


def test_the_read_position_never_runs_ahead():
    for args in [a for a, w, _ in CLASSES if w[0] == "wide"]:
        flt = DS.Filter(*args)
        j = 2 ** 24
        exact, fixed = j * flt.M / flt.L, j * flt.step / 2 ** 32
        assert 0 <= exact - fixed <= 2 ** -8


# ---------------------------------------------------------------------------------------------------------------- the case list

def test_case_list_reaches_what_the_kernel_can_get_wrong():
    cases = DS.cases()
    assert sorted((c.channels, c.frames, c.mix) for c in cases if c.rate == DS.RATE) == sorted((c, t, m) for c in (1, 2) for t in DS.FRAMES for m in (False, True))
    seen = set()
    for c in cases:
        kinds = set()
        for k in range(len(c.windows)):
            flt, f = c.filter(k), c.windows[k][0]
            fr, n = c.frames_in(k), c.frames_out(k)
            kinds.add("away" if flt is None and f < len(DR.files()) else "zero" if not fr else flt.kind)
            if flt is None or flt.kind != "wide" or not fr:
                continue
            ck = DR.files()[f].channels
            assert c.windows[k][1] % ck == 0 and c.windows[k][2] % ck == 0 and flt.n_out(c.windows[k][2] // ck) <= c.frames
            layout = "mono" if c.channels == 1 else "stereo"
            seen.add((layout, "converts" if ck != c.channels else "own"))
            base, p, w, frac = DS.wide_positions(flt, n)
            if flt.L > flt.M and ((p == flt.P - 1) & (w >= 32000)).any():
                seen.add("the last phase pair, w >= 32000")
            if (frac == 0).any():
                seen.add("frac == 0")
            if (frac[1:] == 0).any():
                seen.add("frac == 0 behind frame 0")
            if flt.c == 8 and n > DS.UNIT // 2 + 8 and DS.passes_of_a_unit(flt, 1) > 1:
                seen.add("c == 8 in two passes, %s" % layout)
                assert DS.passes_of_a_unit(flt, 1 if c.channels == 1 else 2) == 2
            if c.frames == 2100 and 8 < n * c.channels % DS.UNIT < DS.UNIT - 8 and n < c.frames - 8:
                seen.add("ends inside a unit")
            if c.frames == 2100 and n * c.channels > DS.UNIT + 8:
                seen.add("two units")
            seen.add(("c", flt.c))
        if c.rate == DS.RATE:
            assert kinds == {"wide", "exact", "none", "zero", "away"}, (c.name, kinds)
        else:
            assert kinds >= {"wide", "exact", "away"}, (c.name, kinds)
        assert len({c.filter(k).key for k in range(len(c.windows)) if c.filter(k) and c.filter(k).key is not None}) <= 16
    want = {(l, m) for l in ("mono", "stereo") for m in ("converts", "own")} | {("c", 64), ("c", 63), ("c", 32), ("c", 31), ("c", 8)}
    want |= {"the last phase pair, w >= 32000", "frac == 0", "frac == 0 behind frame 0", "c == 8 in two passes, mono", "c == 8 in two passes, stereo",
             "ends inside a unit", "two units"}
    assert seen >= want, want - seen


def test_expected_rows_follow_the_formula():
    """the vectorised model against the contract's lines spelled out output by output, on wide rows of every table"""
    done = set()
    for c in DS.cases():
        if c.frames in (2100, 37):
            continue
        rows = c.rows(False)
        for k in range(len(c.windows)):
            flt = c.filter(k)
            if flt is None or flt.kind != "wide" or (flt.c, c.channels) in done or c.frames_in(k) < 20:
                continue
            done.add((flt.c, c.channels))
            f, first, count = c.windows[k]
            q = DS.filter_of(f, c.rate, c.speeds[k])[1]
            x = DR.planes_of(f, first, c.delivers(k), c.channels)
            fr = x.shape[1]
            for e in range(0, min(c.row, 400)):
                j, ch = e // c.channels, e % c.channels
                want = 0
                if j < -(-fr * flt.L // flt.M):
                    X = j * flt.step
                    base, frac = X >> 32, X & 0xFFFFFFFF
                    p, w = frac >> (32 - flt.b), (frac >> (17 - flt.b)) & 32767
                    a0 = sum(int(q[p, t]) * int(x[ch, base - flt.Wd + 1 + t]) for t in range(flt.K) if 0 <= base - flt.Wd + 1 + t < fr)
                    a1 = sum(int(q[p + 1, t]) * int(x[ch, base - flt.Wd + 1 + t]) for t in range(flt.K) if 0 <= base - flt.Wd + 1 + t < fr)
                    want = min(max((a0 + (((a1 - a0) * w) >> 15) + 8192) >> 14, -32768), 32767)
                assert rows[k, e] == want, (c.name, k, e)
    assert {c for c, _ in done} >= {64, 63, 32, 31, 8}


# ---------------------------------------------------------------------------------------------------------------- the host code, sanitized

def test_layout_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "speed_layout")
    csrc = os.path.join(ROOT, "libacm_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "speed_layout.cpp")] + \
          [os.path.join(csrc, f) for f in ("acm_resample_layout.cpp", "acm_dense_layout.cpp", "acm_window_layout.cpp", "acm_kernel_geo.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, "-o", exe] + src + ["-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and "sanitize" in r.stdout and "cannot find" in r.stdout:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


# ---------------------------------------------------------------------------------------------------------------- the kernel's code

@pytest.fixture(scope="module")
def kernel_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "acm_dense_speed.s"
    cmd = [_build.HIPCC, "-O3", "-std=c++17", "--offload-arch=" + _build.GFX, "-I", _build.INC, "-I", _build.CSRC,
           "--cuda-device-only", "-S", "-o", str(out), os.path.join(_build.CSRC, "acm_dense_speed.hip")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return out.read_text()


def test_kernel_has_no_scratch_and_two_workgroups_a_cu(kernel_asm):
    """all six builds: no private segment, 64512 bytes of LDS (two workgroups in a CU's 160 KB), 16-byte global loads and stores, LDS
    accesses and no flat, buffer or scratch access"""
    bodies = {}
    for m in re.finditer(r"^(_ZN\S*acm_dense_speed\S*):", kernel_asm, re.M):
        bodies[m.group(1)] = kernel_asm[m.end():kernel_asm.index(".Lfunc_end", m.end())]
    assert len(bodies) == 6, sorted(bodies)
    for name, body in bodies.items():
        ops = re.findall(r"^\s+((?:global|flat|scratch|buffer|ds)_\w+)", body, re.M)
        assert ops.count("global_load_dwordx4") >= 2 and ops.count("global_store_dwordx4") >= 2, (name, sorted(set(ops)))
        assert any(o.startswith("ds_") for o in ops) and not [o for o in ops if o.startswith(("flat_", "scratch_", "buffer_"))], (name, sorted(set(ops)))
        meta = re.search(r"\.name:\s+%s\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)" % re.escape(name), kernel_asm)
        assert meta and int(meta.group(1)) == 0, name
        desc = kernel_asm[kernel_asm.index(".amdhsa_kernel " + name):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc) and re.search(r"\.amdhsa_group_segment_fixed_size 64512\b", desc), name
