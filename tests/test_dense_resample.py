"""Dense crop batches over files of several sample rates without a GPU: ACM_DENSE_RESAMPLE in the device-free half of
acm_batch_decode_windows_dense (libacm_amd/csrc/acm_dense_layout.cpp, acm_resample_layout.cpp), the case list of tests/dense_resample.py,
and the code the compiler makes of the filtering gather kernel (libacm_amd/csrc/acm_dense_resample.hip).

  * acm_dense_resample_taps() against the contract: L, M, K, Wd, every phase sums to 16384 and cannot overflow 32 bits, equal rates
    are one tap, and the table is the numpy design up to how libm and numpy round a double.
  * the model with the library's taps resamples a sine to 60 dB and keeps a constant exactly.
  * acmk_dense_layout_visit() with the flag: the "resample" and "tables" tables, the soft refusals, every refusal of a whole call, and
    what the flag does not change.
  * what the case list reaches, asserted here so that the GPU tests over the same list cannot pass vacuously.
  * acm_dense_resample.hip compiled to gfx950 assembly: no scratch, 63 KB of LDS, 16-byte global loads and stores."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_crops as DC
import dense_resample as DR
import test_dense_crops as TD
import test_window_layout as WL
from libacm_amd import _build, batch, capi

RS = capi.DENSE_RESAMPLE
RATIOS = [(11025, 22050), (44100, 22050), (16000, 22050), (48000, 11025), (22050, 16000), (8000, 22050), (44100, 48000), (48000, 44100)]
PLAIN_TABLES = ["wins", "rejected", "report", "rows", "totals"]
ALL_ONES = 2 ** 64 - 1


# ---------------------------------------------------------------------------------------------------------------- the taps

@pytest.mark.parametrize("rates", RATIOS, ids=lambda r: "%d_%d" % r)
def test_taps_are_the_contracts(rates):
    L, M, K, Wd, q = capi.dense_resample_taps(*rates)
    g = np.gcd(*rates)
    assert (L, M) == (rates[1] // g, rates[0] // g) and Wd == (8 if L >= M else -(-8 * M // L)) and K == 2 * Wd
    assert (L, M, K, Wd) == DR.ratio(*rates) and L * K <= 16384 and q.shape == (L, K) and q.dtype == np.int16
    q = q.astype(np.int64)
    assert (q.sum(axis=1) == 16384).all()
    assert np.abs(q).sum(axis=1).max() < 65536
    # the numpy design: libm and numpy may round a double apart, by one; the tap that makes up the sum follows the others
    want = DR.design(*rates)[4]
    off = np.abs(q - want)
    fix = want.argmax(axis=1)
    others = off.copy()
    others[np.arange(L), fix] = 0
    assert others.max() <= 1
    assert (off[np.arange(L), fix] <= 1 + (others != 0).sum(axis=1)).all()
    assert capi.dense_resampled_frames(1000, *rates) == -(-1000 * L // M) and capi.dense_resampled_frames(0, *rates) == 0


def test_table_sizes_of_the_contract():
    sizes = {r: capi.dense_resample_taps(*r)[:4] for r in RATIOS}
    assert sizes[(22050, 16000)] == (320, 441, 24, 12) and sizes[(8000, 22050)] == (441, 160, 16, 8) and sizes[(48000, 11025)] == (147, 640, 70, 35)
    assert sizes[(11025, 22050)] == (2, 1, 16, 8) and sizes[(44100, 22050)] == (1, 2, 32, 16) and sizes[(16000, 22050)] == (441, 320, 16, 8)


def test_equal_rates_are_one_tap():
    L, M, K, Wd, q = capi.dense_resample_taps(22050, 22050)
    assert (L, M, K, Wd) == (1, 1, 16, 8) and q[0, Wd - 1] == 16384 and np.count_nonzero(q) == 1
    assert capi.dense_resampled_frames(12345, 22050, 22050) == 12345


def test_ratios_that_are_not_supported():
    for rates in ((22051, 22050), (0, 22050), (22050, 0), (22050, 2450), (22050, 1)):      # a table too large, no rate, M > 8 L
        with pytest.raises(ValueError):
            capi.dense_resample_taps(*rates)
        assert capi.dense_resampled_frames(100, *rates) is None
    assert capi.dense_resample_taps(22048, 2756)[1] == 8                                    # M == 8 L
    # the sizes alone, and a table that does not fit
    n = [C.c_uint32() for _ in range(4)]
    assert capi.lib().acm_dense_resample_taps(16000, 22050, *[C.byref(v) for v in n], None, 0) == 0 and [v.value for v in n] == [441, 320, 16, 8]
    room = np.zeros(441 * 16, np.int16)
    assert capi.lib().acm_dense_resample_taps(16000, 22050, None, None, None, None, room.ctypes.data, room.size - 1) == capi.ERR_ARG and not room.any()
    assert capi.lib().acm_dense_resample_taps(16000, 22050, None, None, None, None, room.ctypes.data, room.size) == 0 and room.any()
    assert batch.source_frames(2100, 44100, 22050) == 4200 and batch.source_frames(2100, 16000, 22050) == 1523 and batch.source_frames(64, 22050, 22050) == 64


# ---------------------------------------------------------------------------------------------------------------- quality

@pytest.mark.parametrize("rates", [(11025, 22050), (44100, 22050), (22050, 16000)], ids=lambda r: "%d_%d" % r)
def test_a_sine_comes_out_a_sine(rates):
    """1 kHz, amplitude 20000, 4000 frames, against the sine sampled at the target rate, 200 frames dropped at either end: 60 dB.
    Measured with this definition: 73.1, 66.9 and 67.3 dB; the margin is for taps that differ by the 1 allowed above"""
    ri, ro = rates
    table = DR.taps(ri, ro)
    x = np.rint(20000 * np.sin(2 * np.pi * 1000 * np.arange(4000) / ri)).astype(np.int64)
    y, _ = DR.filter_frames(x, table)
    assert y.size == DR.n_out(4000, table[0], table[1])
    want = 20000 * np.sin(2 * np.pi * 1000 * np.arange(y.size) / ro)
    err = (y - want)[200:-200]
    snr = 10 * np.log10((want[200:-200] ** 2).sum() / (err ** 2).sum())
    print("%d -> %d: %.1f dB" % (ri, ro, snr))
    assert snr >= 60


@pytest.mark.parametrize("rates", RATIOS, ids=lambda r: "%d_%d" % r)
def test_a_constant_stays_what_it_is(rates):
    table = DR.taps(*rates)
    y, _ = DR.filter_frames(np.full(1500, 12345), table)
    edge = 2 * table[3] * table[0] // table[1] + 2                  # outputs whose taps reach over an end of the crop
    assert (y[edge:-edge] == 12345).all() and y.size > 4 * edge


# ---------------------------------------------------------------------------------------------------------------- the layout

def _lib():
    L = capi.lib()
    L.acmk_dense_layout_visit.argtypes = [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, WL.VISIT, C.c_void_p]
    return L


def call(items, wins, frames, channels, dense_flags=RS, rate=DR.RATE, reserved=0, parse=capi.PARSE_HOST, f32=False, final_words=None, short_opts=False):
    """tests/test_dense_crops.py::call with every item's own rate and the two fields behind acm_dense_opts.flags.  short_opts: the
    16-byte acm_dense_opts of a caller that knows no such fields, poison where they would be"""
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
    win3 = np.array(wins, dtype=np.uint64).reshape(-1)
    opts = capi.BatchOpts(0, capi.FMT_S16LE, 4, 0, parse, capi.BATCH_PCM_F32 if f32 else 0, TD.FAKE_PTR, nwin * frames * channels, None)
    if short_opts:
        raw = np.full(3, 0xEEEEEEEEEEEEEEEE, np.uint64)
        raw[0], raw[1] = frames, channels | dense_flags << 32
        dense = C.c_void_p(raw.ctypes.data)
    else:
        dense = C.byref(capi.DenseOpts(frames, channels, dense_flags, rate, reserved))
    final = None if final_words is None else np.array(final_words, dtype=np.uint64)
    tables = {}

    def visit(_ctx, name, data, elem_bytes, count):
        assert name.decode() not in tables and elem_bytes % 8 == 0
        tables[name.decode()] = np.frombuffer(C.string_at(data, elem_bytes * count), dtype="<u8").reshape(count, elem_bytes // 8).copy()
    rc = _lib().acmk_dense_layout_visit(info, length.ctypes.data, ok.ctypes.data, end_status.ctypes.data, whole.ctypes.data, marks, blocks.ctypes.data,
                                        n, win3.ctypes.data if nwin else None, nwin, C.byref(opts), dense,
                                        final.ctypes.data if final is not None else None, WL.VISIT(visit), None)
    tot = dict(zip(TD.TOTALS, tables["totals"].reshape(-1).astype(np.int64).tolist()))
    assert tot["rc"] == rc
    return rc, tables, tot


@pytest.fixture(scope="module")
def items():
    return [DR.layout_item(f) for f in DR.files()]


def with_rate(item, rate):
    """the item with another rate in its header - the visitor takes what the probe would not"""
    from types import SimpleNamespace
    return SimpleNamespace(**{**vars(item), "info": SimpleNamespace(**{**vars(item.info), "rate": rate})})


@pytest.mark.parametrize("parse", [capi.PARSE_HOST, capi.PARSE_DEVICE], ids=["host", "device"])
def test_layout_tables(items, parse):
    for case in DR.cases():
        flags = RS | (capi.DENSE_MIX if case.mix else 0)
        rc, got, tot = call(items, case.windows, case.frames, case.channels, dense_flags=flags, parse=parse)
        assert rc == 0 and list(got) == PLAIN_TABLES[:-1] + (["mix"] if case.mix else []) + ["resample", "tables", "totals"], case.name
        tabs = TD.signed(got["tables"])
        assert sorted(t[0] for t in tabs) == [11025, 16000, 44100]
        at = 0
        for ri, L, M, K, Wd, off in tabs:                               # in the order of their first window, 16-byte lines apart
            assert (L, M, K, Wd) == DR.ratio(ri, DR.RATE) and off == at and off % 8 == 0
            at += -(-L * K // 8) * 8
        n = len(case.windows)
        assert tot["table_bytes"] == 16 * n + 32 * n + 2 * at
        res = got["resample"]
        assert res.shape == (n + 1, 5) and res[n].tolist() == [1, 0, 0, 0, 0]
        nblocks = 0
        for k, (f, first, count) in enumerate(case.windows):
            words, status, nb = case.expect(k)
            nblocks += nb
            assert tuple(TD.signed(got["report"])[k][:2]) == (status, words) and words == case.delivers(k), (case.name, k)
            L, M, tid, frames_out, bad = res[k].tolist()
            # (a window turned away for its channel count is not asked for its rate)
            assert bad == int(f == 8 and (case.mix or case.channels == 1))
            assert frames_out == case.frames_out(k) <= case.frames, (case.name, k)
            if case.filtered(k) and words:
                assert (L, M) == DR.table_of(f)[:2] and tabs[tid][0] == DR.rate_of(f)
            else:
                assert (L, M, tid) == ((0, 0, ALL_ONES) if bad else (1, 1, ALL_ONES))
            assert int(got["rejected"][k][0]) == int(f < len(DR.files()) and DR.turned_away(f, case.channels, case.mix))
        assert tot["blocks_parsed"] == nblocks


def test_rates_the_filter_does_not_take_are_turned_away_softly(items):
    """22051 Hz and, through the visitor alone, rate 0: words 0, ERR_ARG, nothing parsed; the other windows as if they were not there"""
    its = items + [with_rate(items[4], 0)]
    good = [(0, 8, 32), (4, 16, 128), (2, 3, 64)]
    rc, alone, tot0 = call(its, good, 64, 1)
    rc, got, tot = call(its, [good[0], (8, 5, 64), good[1], (12, 7, 64), (8, 0, 0), good[2]], 64, 1)
    assert rc == 0 and tot["blocks_parsed"] == tot0["blocks_parsed"] > 0
    rep, res = TD.signed(got["report"]), got["resample"].tolist()
    for k in (1, 3, 4):
        assert rep[k][:2] == (capi.ERR_ARG, 0) and res[k] == [0, 0, ALL_ONES, 0, 1] and int(got["rejected"][k][0]) == 1 and int(got["wins"][k][2]) == 0
        assert TD.signed(got["rows"])[k] == (0, 0)
    assert [rep[k][:2] for k in (0, 2, 5)] == [r[:2] for r in TD.signed(alone["report"])] == [(0, 32), (0, 128), (0, 64)]
    assert [res[k] for k in (0, 2, 5)] == alone["resample"].tolist()[:3] == [[2, 1, 0, 64, 0], [1, 2, 1, 64, 0], [1, 1, ALL_ONES, 64, 0]]
    # such a window is checked as a row of the batch's own rate: T frames at most
    assert call(its, good + [(8, 0, 65)], 64, 1)[0] == capi.ERR_ARG and call(its, good + [(12, 0, 65)], 64, 1)[0] == capi.ERR_ARG


def test_refusals_of_a_whole_call(items):
    wins, T = [(2, 8, 32), (4, 16, 128), (0, 4, 32), (5, 4, 256)], 64
    MIX = capi.DENSE_MIX
    assert call(items, wins, T, 1, dense_flags=RS | MIX)[0] == 0
    for what, kw in (("rate == 0", dict(rate=0)), ("reserved != 0", dict(reserved=1)), ("unknown flag 2", dict(dense_flags=RS | MIX | 2)),
                     ("unknown flag 8", dict(dense_flags=RS | MIX | 8)), ("unknown flag 0x80000001", dict(dense_flags=0x80000001))):
        rc, tables, tot = call(items, wins, T, 1, **{"dense_flags": RS | MIX, **kw})
        assert rc == capi.ERR_ARG and list(tables) == ["totals"], what
    for what, bad, ch in (("a 44100 Hz window one frame too long", (4, 0, 129), 1), ("an 11025 Hz window one frame too long", (0, 0, 33), 1),
                          ("a 16000 Hz window one frame too long", (6, 0, 47), 1), ("a stereo 44100 Hz window one frame too long", (5, 0, 258), 1),
                          ("a 22050 Hz window one frame too long", (2, 0, 65), 1), ("far too long", (4, 0, 1 << 40), 1),
                          ("odd first_word on a stereo item", (5, 3, 8), 1), ("odd max_words on a stereo item", (1, 4, 7), 2),
                          ("odd first_word of a stereo window that asks for nothing", (7, 1, 0), 1)):
        rc, tables, tot = call(items, wins[:1] + [bad] + wins[1:], T, ch, dense_flags=RS | MIX)
        assert rc == capi.ERR_ARG and list(tables) == ["totals"], what
    for what, good, ch in (("the longest 44100 Hz window", (4, 1, 128), 1), ("the longest 11025 Hz window", (0, 3, 32), 1),
                           ("the longest 16000 Hz window", (6, 5, 46), 1), ("the longest stereo 44100 Hz window", (5, 2, 256), 2)):
        rc, tables, tot = call(items, wins[:1] + [good] + wins[1:], T, ch, dense_flags=RS | MIX)
        assert rc == 0 and int(tables["resample"][1][3]) == T, what
    assert DR.n_out(46, 441, 320) == 64 and DR.n_out(47, 441, 320) == 65 and batch.source_frames(64, 16000, 22050) == 46
    # 16 distinct ratios are taken, the 17th is not
    rates = [22050 * a // b for a, b in ((1, 2), (2, 1), (1, 3), (3, 1), (2, 3), (3, 2), (1, 5), (5, 1), (2, 5), (5, 2), (3, 5), (5, 3), (1, 6), (1, 7),
                                         (7, 1), (2, 7), (7, 2))]
    assert len(set(rates)) == 17 and all(DR.ratio(r, DR.RATE) for r in rates)
    its = [with_rate(items[2], r) for r in rates]
    rc, tables, tot = call(its, [(k, 0, 8) for k in range(16)], T, 1)
    assert rc == 0 and tables["tables"].shape == (16, 6)
    assert call(its, [(k, 0, 8) for k in range(17)], T, 1)[0] == capi.ERR_ARG
    assert call(its, [(k % 16, 0, 8) for k in range(40)], T, 1)[0] == 0
    # frames beyond 2^40 are not taken with the flag
    assert call(items, [], 1 << 40, 1)[0] == capi.ERR_ARG and call(items, [], (1 << 40) - 1, 1)[0] == 0


def test_without_the_flag_and_over_one_rate_nothing_changes(items):
    """the flag unset - also in the 16-byte acm_dense_opts of a caller that knows no rate - and the flag over files that are all at the
    batch's rate: the tables of tests/test_dense_crops.py::call, table for table, byte for byte"""
    plain_items = [DC.layout_item(f) for f in DR.files()]               # without a rate: TD.call says 22050 for every file
    for C_, T in ((1, 64), (2, 37)):
        own = [f for f in (2, 3) if DR.files()[f].channels == C_][0]
        W = DR.files()[own].words
        wins = [(own, 8 * C_, T * C_), (own, 3 * C_, 5 * C_), (10, 0, 0), (own, W - 6 * C_, T * C_), (99, 0, 2 * C_), (5 - own, 4, 36)]
        for planar in (0, 1):
            for parse in (capi.PARSE_HOST, capi.PARSE_DEVICE):
                for mix in (0, capi.DENSE_MIX):
                    rc0, want, tot0 = TD.call(plain_items, wins, T, C_, dense_flags=planar | mix, parse=parse)
                    rc1, unset, tot1 = call(items, wins, T, C_, dense_flags=planar | mix, rate=0xEEEEEEEE, reserved=0xEEEEEEEE, parse=parse)
                    rc2, short, tot2 = call(items, wins, T, C_, dense_flags=planar | mix, parse=parse, short_opts=True)
                    rc3, flagged, tot3 = call(items, wins, T, C_, dense_flags=planar | mix | RS, parse=parse)
                    assert rc0 == rc1 == rc2 == rc3 == 0 and tot0 == tot1 == tot2 == tot3
                    assert list(want) == list(unset) == list(short) and list(flagged) == list(want)[:-1] + ["resample", "tables", "totals"]
                    for name in want:
                        assert want[name].tobytes() == unset[name].tobytes() == short[name].tobytes() == flagged[name].tobytes(), (name, planar, mix)
                    assert flagged["tables"].size == 0 and flagged["resample"][-1].tolist() == [0, 0, 0, 0, 0]
                    assert all(r[:3] == [1, 1, ALL_ONES] for r in flagged["resample"][:-1].tolist())


def test_windows_staging_left_nothing_of(items):
    """what staging left decides: with every filtered window turned away mid-call no row is filtered"""
    case = DR.cases()[0]
    rc, before, _ = call(items, case.windows, case.frames, 1, dense_flags=RS | capi.DENSE_MIX)
    final = [int(r[1]) for r in before["report"]]
    hit = [k for k in range(len(final)) if final[k] and case.filtered(k)]
    assert len(hit) > 20
    for k in hit[1:]:
        final[k] = 0
    rc, got, tot = call(items, case.windows, case.frames, 1, dense_flags=RS | capi.DENSE_MIX, final_words=final)
    assert rc == 0 and got["resample"][-1][0] == 1 and [k for k in range(len(final)) if got["resample"][k][0] > 1 or got["resample"][k][1] > 1] == hit[:1]
    final[hit[0]] = 0
    rc, got, tot = call(items, case.windows, case.frames, 1, dense_flags=RS | capi.DENSE_MIX, final_words=final)
    assert rc == 0 and got["resample"][-1][0] == 0


# ---------------------------------------------------------------------------------------------------------------- the case list

def test_case_list_reaches_what_the_kernel_can_get_wrong():
    cases = DR.cases()
    assert sorted((c.channels, c.frames, c.mix) for c in cases) == sorted((c, t, m) for c in (1, 2) for t in DR.FRAMES for m in (False, True))
    residues = {}
    for c in cases:
        rows = c.rows(False)
        kinds = [c.filtered(k) for k in range(len(c.windows))]
        changes = sum(a != b for a, b in zip(kinds, kinds[1:]))
        assert changes >= min(kinds.count(True), kinds.count(False)), (c.name, changes)
        lengths, seen, what = {}, set(), set()
        for k, (f, first, count) in enumerate(c.windows):
            seen.add(f)
            if not c.filtered(k):
                continue
            src, table = DR.files()[f], DR.table_of(f)
            ck, F = src.channels, DR.longest(f, c.frames)
            assert first % ck == 0 and count % ck == 0 and count // ck <= F and DR.n_out(count // ck, table[0], table[1]) <= c.frames
            lengths.setdefault(f, set()).add(count // ck)
            fr = c.delivers(k) // ck
            if fr >= 9:
                residues.setdefault((src.info.rate, ck), set()).add(first % 8)
            if first >= src.words:
                what.add("behind the end")
            elif c.delivers(k) < count:
                what.add("clipped by the end" if src.end_status == 0 else "clipped by a stream that breaks off")
            if fr and first // src.st.block_len != (first + fr * ck - 1) // src.st.block_len:
                what.add("across a block boundary")
            # a full row ends with the row: the last frame is the window's, not padding
            if count // ck == F and fr == F:
                assert c.frames_out(k) in (c.frames, c.frames - 1)
        assert seen == set(range(12)) | {99}, c.name
        # (the file that breaks off is mono: turned away by a stereo batch without ACM_DENSE_MIX)
        broken = {"clipped by a stream that breaks off"} if c.mix or c.channels == 1 else set()
        assert what == {"behind the end", "clipped by the end", "across a block boundary"} | broken, (c.name, what)
        for f, got in lengths.items():
            if f != 11:
                Wd, F = DR.table_of(f)[3], DR.longest(f, c.frames)
                assert {0, 1, 2, Wd - 1, F - 1, F} <= got, (c.name, f, sorted(got))
        if c.frames == 2100:
            # a row of two units: outputs on either side of element 2048 (+ up to 7 of the head), at a source base that is no multiple of 8
            full = [k for k in range(len(c.windows)) if c.filtered(k) and c.frames_out(k) * (1 if c.channels == 1 else 2) > 2048 + 8]
            assert len(full) >= 6
            bases = {2048 // c.channels * DR.table_of(c.windows[k][0])[1] // DR.table_of(c.windows[k][0])[0] % 8 for k in full}
            assert bases - {0}, c.name
    for rate in (11025, 44100, 16000):
        assert residues[(rate, 1)] == set(range(8)) and residues[(rate, 2)] == {0, 2, 4, 6}, (rate, residues)


def test_rows_saturate_and_round():
    """among the filtered rows: outputs the clamp holds at either end of int16, and sums whose rounding bit decides"""
    high = low = half = 0
    for c in DR.cases():
        c.rows(False)
        assert c.accs
        for acc in c.accs:
            y = (acc + 8192) >> 14
            high += int((y > 32767).sum())
            low += int((y < -32768).sum())
            half += int(((acc & 16383) == 8192).sum())
    assert high > 10 and low > 10 and half > 0, (high, low, half)
    assert any((c.rows(False) == 32767).any() and (c.rows(False) == -32768).any() for c in DR.cases())


def test_expected_rows_follow_the_formula():
    """the vectorised model against the contract's three lines spelled out output by output, on a sample of rows of every kind"""
    rng = np.random.default_rng(0xD5)
    for c in DR.cases():
        if c.frames == 2100:
            continue
        C_, T = c.channels, c.frames
        for planar in (False, True):
            rows = c.rows(planar)
            picked = [k for k in rng.permutation(len(c.windows)).tolist() if c.filtered(k) and c.delivers(k)][:6]
            for k in picked:
                f, first, count = c.windows[k]
                L, M, K, Wd, q = DR.table_of(f)
                x = DR.planes_of(f, first, c.delivers(k), C_)
                fr = x.shape[1]
                for e in range(c.row):
                    j, ch = (e % T, e // T) if planar else (e // C_, e % C_)
                    want = 0
                    if j < DR.n_out(fr, L, M):
                        base, ph = j * M // L, j * M % L
                        acc = sum(int(q[ph, t]) * int(x[ch, base - Wd + 1 + t]) for t in range(K) if 0 <= base - Wd + 1 + t < fr)
                        want = min(max((acc + 8192) >> 14, -32768), 32767)
                    assert rows[k, e] == want, (c.name, planar, k, e)


# ---------------------------------------------------------------------------------------------------------------- the kernel's code

@pytest.fixture(scope="module")
def kernel_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "acm_dense_resample.s"
    cmd = [_build.HIPCC, "-O3", "-std=c++17", "--offload-arch=" + _build.GFX, "-I", _build.INC, "-I", _build.CSRC,
           "--cuda-device-only", "-S", "-o", str(out), os.path.join(_build.CSRC, "acm_dense_resample.hip")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return out.read_text()


def test_kernel_has_no_scratch_and_two_workgroups_a_cu(kernel_asm):
    """all six builds: no private segment, 64512 bytes of LDS (two workgroups in a CU's 160 KB), 16-byte global loads and stores, LDS
    accesses and no flat, buffer or scratch access"""
    bodies = {}
    for m in re.finditer(r"^(_ZN\S*acm_dense_resample\S*):", kernel_asm, re.M):
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
