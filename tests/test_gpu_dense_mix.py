"""acm_batch_decode_windows_dense with ACM_DENSE_MIX on the GPU (include/acm_hip.h; libacm_amd/csrc/acm_batch_windows.cpp,
acm_dense_mix.hip): mono and stereo files as the rows of one tensor.

Every call writes into the middle of a poisoned buffer with a guard row on either side (tests/test_gpu_dense_crops.py::run): the guards
must keep the poison and the rows must be the expected ones exactly.  The handle's fill mode is on (helpers): a gather that reads a place
the synthesis did not write shows up as 0xA5A5.

Expected rows: tests/dense_mix.py (the oracle's whole-file decode and the contract's table; tests/test_dense_mix.py holds the case list
to what it has to reach).  Every call here sets dense flag 4, which the library refused before it knew ACM_DENSE_MIX."""
import numpy as np
import pytest

import dense_crops as DC
import dense_mix as DM
from helpers import make_stream
from libacm_amd import capi
from test_gpu_dense_crops import BOTH, POISON, data_and_index, run, same

pytestmark = pytest.mark.gpu

_plain = {}


def windows_call(dev, case, parse):
    """(statuses, words, blocks_parsed) of acm_batch_decode_windows for the case's windows: once per case and parser"""
    key = (case.name, parse)
    if key not in _plain:
        files, index = data_and_index()
        cap = capi.batch_window_pcm_words(files, case.windows)
        d = dev.malloc(max(cap, 1) * 2)
        try:
            st, words, _, _, tm = capi.batch_decode_windows_device(dev, files, index, case.windows, d, cap, parse=parse, threads=4)
        finally:
            dev.free(d)
        _plain[key] = (st, words, tm.blocks_parsed)
    return _plain[key]


def first_difference(got, want_i16, f32):
    want = DC.as_f32(want_i16).view(np.uint32) if f32 else want_i16.view(np.uint16)
    bad = np.nonzero(got != want)[0]
    return "%d of %d elements differ, the first at %d" % (bad.size, got.size, int(bad[0]))


# ---------------------------------------------------------------------------------------------------------------- expected rows

@pytest.mark.parametrize("parse", BOTH, ids=["host", "device"])
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("case", DM.cases(), ids=lambda c: c.name)
def test_expected_rows(dev, case, f32, planar, parse):
    files, index = data_and_index()
    got, st, words, tm = run(dev, files, index, case.windows, case.frames, case.channels, planar, f32, parse, mix=True)
    want = case.rows(planar)
    nblocks = 0
    for k in range(len(case.windows)):
        w, status, nb = case.expect(k)
        nblocks += nb
        assert (words[k], st[k]) == (w, status), (k, case.windows[k], words[k], st[k], w, status)
        assert same(got[k], want[k], f32), "row %d, window %r, mode %d: %s" % (k, case.windows[k], case.mode(k, planar),
                                                                                 first_difference(got[k], want[k], f32))
    assert tm.blocks_parsed == nblocks and tm.samples == sum(words)
    assert (tm.device_parsed > 0) == (parse == capi.PARSE_DEVICE)
    # words and status are the windows call's for the same windows, and so are the blocks parsed
    w_st, w_words, w_blocks = windows_call(dev, case, parse)
    assert st == w_st and words == w_words and tm.blocks_parsed == w_blocks


# ---------------------------------------------------------------------------------------------------------------- an odd element offset

@pytest.mark.parametrize("parse", BOTH, ids=["host", "device"])
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("case", [c for c in DM.cases() if c.channels == 2], ids=lambda c: c.name)
def test_interleaved_stereo_batch_one_element_off_a_line(dev, case, f32, parse):
    """the tensor begins DM.ODD_SHIFT = 1 element behind a 16-byte line: the body of every row then starts on the second copy of a
    sample, where an up-mixed vector needs 9 source samples (tests/test_dense_mix.py asserts that the rows of these cases get there, at
    every source residue).  Guards: the element in front of the tensor, a row in front of that and a row behind"""
    files, index = data_and_index()
    n, R = len(case.windows), case.row
    unit, dt = (4, np.uint32) if f32 else (2, np.uint16)
    total = (n + 2) * R + DM.ODD_SHIFT
    d = dev.malloc(total * unit)
    try:
        assert d % 256 == 0
        dev.memset(d, POISON, total * unit)
        st, words, tm = capi.batch_decode_windows_dense(dev, files, index, case.windows, d + (R + DM.ODD_SHIFT) * unit, n * R, case.frames, channels=2,
                                                        planar=False, f32=f32, parse=parse, threads=4, mix=True)
        raw = np.zeros(total, dtype=dt)
        dev.download(raw, d)
    finally:
        dev.free(d)
    poison = np.frombuffer(bytes([POISON]) * unit, dtype=dt)[0]
    assert (raw[:R + DM.ODD_SHIFT] == poison).all(), "the call wrote in front of its tensor"
    assert (raw[total - R:] == poison).all(), "the call wrote behind its tensor"
    got, want = raw[R + DM.ODD_SHIFT:total - R].reshape(n, R), case.rows(False)
    for k in range(n):
        assert (words[k], st[k]) == case.expect(k)[:2]
        assert same(got[k], want[k], f32), "row %d, window %r, mode %d: %s" % (k, case.windows[k], case.mode(k, False),
                                                                                 first_difference(got[k], want[k], f32))


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_refused_calls_write_nothing(dev):
    files, index = data_and_index()
    wins, T = [(0, 8, 32), (2, 16, 64), (1, 4, 128)], 64
    for what, bad, channels in (("odd first_word on a stereo item, C = 1", (1, 3, 8), 1), ("max_words > 2T on a stereo item, C = 1", (3, 0, 2 * T + 2), 1),
                                ("max_words > T on a mono item, C = 2", (0, 0, T + 1), 2), ("odd max_words on a stereo item, C = 1", (5, 0, 7), 1)):
        windows = wins[:1] + [bad] + wins[1:]
        n, R = len(windows), T * channels
        d = dev.malloc((n + 2) * R * 2)
        try:
            dev.memset(d, POISON, (n + 2) * R * 2)
            res = capi.batch_decode_windows_dense(dev, files, index, windows, d + 2 * R, n * R, T, channels=channels, mix=True, check=False, threads=2)
            raw = np.zeros((n + 2) * R, np.uint16)
            dev.download(raw, d)
        finally:
            dev.free(d)
        assert res[-1] == capi.ERR_ARG, (what, res[-1])
        assert (raw == POISON * 0x101).all(), what
    # the accepted call next to them: 2T samples of a stereo item under C = 1
    got, st, words, tm = run(dev, files, index, wins, T, 1, False, False, capi.PARSE_HOST, mix=True)
    assert st == [0, 0, 0] and words == [32, 64, 128]
    assert all(same(got[k], DM.row_of(*w, 1, T, False), False) for k, w in enumerate(wins))


# ---------------------------------------------------------------------------------------------------------------- one channel count

@pytest.mark.parametrize("case", DC.cases(), ids=lambda c: c.name)
def test_the_flag_over_one_channel_count_changes_nothing(dev, case):
    """a batch of one channel count with the flag set: bit for bit the call without the flag"""
    files, index = data_and_index()
    wins = [w for k, w in enumerate(case.windows) if not case.rejected(k)]
    for f32, planar, parse in ((False, False, capi.PARSE_HOST), (True, True, capi.PARSE_DEVICE), (False, True, capi.PARSE_DEVICE), (True, False, capi.PARSE_HOST)):
        plain, st0, words0, tm0 = run(dev, files, index, wins, case.frames, case.channels, planar, f32, parse)
        mixed, st1, words1, tm1 = run(dev, files, index, wins, case.frames, case.channels, planar, f32, parse, mix=True)
        assert np.array_equal(plain, mixed) and plain.any()
        assert st0 == st1 and words0 == words1 and (tm0.blocks_parsed, tm0.samples, tm0.h2d_bytes) == (tm1.blocks_parsed, tm1.samples, tm1.h2d_bytes)


# ---------------------------------------------------------------------------------------------------------------- turned away during the call

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
def test_a_window_the_stager_rejects_is_a_row_of_zeros_among_converted_rows(dev, f32):
    """tests/test_gpu_dense_crops.py's stale index - the marks of another file of the same shape - in a stereo batch: the two mono files
    are up-mixed, the windows the stager turns away mid-call are rows of zeros with the windows call's status, a stereo file's rows
    between them are copied"""
    a, b = make_stream(9300, 7, 16, 12, mix=1), make_stream(9301, 7, 16, 12, mix=1)
    fa, fb, fc = DC.File(a), DC.File(b), DC.files()[5]
    n = int((fb.marks["bit"][:fa.marks.size] <= 8 * len(a)).sum())
    assert n >= 10
    files, stale, pcm = [a, b, fc.data], [fb.marks[:n].copy(), fb.marks, fc.marks], (fa.pcm, fb.pcm, fc.pcm)
    bl, T = fa.st.block_len, 48
    windows = [(1, 5, T), (0, 3 * bl + 11, T), (2, 40, 2 * T), (1, 2 * bl + 5, 40), (0, 0, T), (0, 7 * bl - 9, 33), (2, 1002, 2 * 9), (1, bl - 7, T),
               (0, 5 * bl + 1, 1), (1, 77, T)]

    def upmixed(k, words, planar):
        f, first, count = windows[k]
        row = np.zeros(2 * T, np.int16)
        src = pcm[f][first:first + words]
        if f == 2:
            row[:words] = src
            return np.ascontiguousarray(row.reshape(T, 2).T).reshape(-1) if planar else row
        if planar:
            row[:words] = row[T:T + words] = src
        else:
            row[0:2 * words:2] = row[1:2 * words:2] = src
        return row

    for parse in BOTH:
        cap = capi.batch_window_pcm_words(files, windows)
        d = dev.malloc(cap * 2)
        try:
            w_st, w_words = capi.batch_decode_windows_device(dev, files, stale, windows, d, cap, parse=parse, threads=4)[:2]
        finally:
            dev.free(d)
        turned_away = [k for k, s in enumerate(w_st) if s != 0 and w_words[k] == 0]
        assert turned_away and all(w_st[k] == 0 for k, w in enumerate(windows) if w[0] != 0)
        for planar in (False, True):
            got, st, words, tm = run(dev, files, stale, windows, T, 2, planar, f32, parse, mix=True)
            assert st == w_st and words == w_words
            for k in range(len(windows)):
                assert words[k] == windows[k][2] or st[k] != 0
                assert same(got[k], upmixed(k, words[k], planar), f32), (k, windows[k], parse, planar)
            assert not got[turned_away].any()


# ---------------------------------------------------------------------------------------------------------------- many rows

@pytest.mark.parametrize("channels,planar,f32", [(1, False, False), (2, False, True), (2, True, False)], ids=["down", "up_interleaved", "up_planar"])
def test_66000_rows(dev, channels, planar, f32):
    """more work than the grid has workgroups, 8 frames a row, the converting and the plain mode alternating row by row: a seeded sample
    of 500 rows, the first and the last"""
    files, index = data_and_index()
    rng = np.random.default_rng([66000, channels, int(planar)])
    n, T = 66000, 8
    src = np.where(np.arange(n) % 2 == 0, rng.choice([0, 2, 4], n), rng.choice([1, 3, 5], n))
    c = np.array([DC.files()[f].channels for f in range(6)])[src]
    frames_in = np.array([DC.files()[f].words for f in range(6)])[src] // c
    first = c * (rng.integers(0, 1 << 30, n) % (frames_in - 1))
    count = c * rng.integers(0, T + 1, n)
    windows = list(zip(src.tolist(), first.tolist(), count.tolist()))
    got, st, words, tm = run(dev, files, index, windows, T, channels, planar, f32, capi.PARSE_AUTO, threads=0, mix=True)
    assert tm.device_parsed > 50000
    picked = [0, 1, n - 2, n - 1] + rng.choice(n, 500, replace=False).tolist()
    assert len({DM.mode_of(windows[k][0], channels, planar) for k in picked}) == 2
    for k in picked:
        f, a, m = windows[k]
        assert words[k] == DM.delivered(f, a, m) and same(got[k], DM.row_of(f, a, m, channels, T, planar), f32), (k, windows[k])
    assert sum(1 for w in words if w) > 50000


# ---------------------------------------------------------------------------------------------------------------- python

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
def test_gpu_decoder_crop_batch_mix(f32):
    """windows in frames over all eight files, whatever their channel count; the front end multiplies by each file's own"""
    import torch
    from libacm_amd import batch
    fs = DC.files()
    files = [f.data for f in fs]
    dec = batch.GpuDecoder(0, parse=capi.PARSE_DEVICE, dtype=torch.float32 if f32 else torch.int16)
    try:
        index = batch.build_index(files, threads=2)
        T = 50
        windows = [(0, 0, T), (1, 37, T), (2, 300, 41), (3, fs[3].words // 2 - 10, T), (4, 3, 20), (5, 511, 1), (6, 9, 0), (7, 0, 5), (5, 900, T),
                   (6, fs[6].words - 20, T), (0, 77, 9), (1, 3, 8)]
        for channels in (1, 2):
            for planar in (True, False):
                batch_t, frames, st = dec.crop_batch(files, windows, T, channels=channels, planar=planar, index=index, mix=True)
                n = len(windows)
                assert batch_t.dtype == dec.dtype and batch_t.is_cuda and tuple(batch_t.shape) == ((n, channels, T) if planar else (n, T, channels))
                got = batch_t.cpu().numpy().reshape(n, -1)
                for k, (f, a, m) in enumerate(windows):
                    c = DM.chans_of(f, channels)
                    want = DM.row_of(f, a * c, m * c, channels, T, planar)
                    assert frames[k] == DM.delivered(f, a * c, m * c) // c
                    assert st[k] == (0 if frames[k] == m else fs[f].end_status), (k, st[k])
                    assert np.array_equal(got[k].view(np.uint8), (DC.as_f32(want) if f32 else want).view(np.uint8)), (k, channels, planar)
                assert sum(frames) == 50 + 50 + 41 + 10 + 20 + 1 + 50 + 20 + 9 + 8
        # without mix the same windows over the files of the other channel count stay rows of zeros
        batch_t, frames, st = dec.crop_batch(files, windows, T, channels=1, index=index)
        assert [st[k] for k in (1, 3, 5, 8, 11)] == [capi.ERR_ARG] * 5 and not batch_t[[1, 3, 5, 8, 11]].any()
    finally:
        dec.dev.close()
