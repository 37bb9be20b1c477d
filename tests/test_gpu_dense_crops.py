"""acm_batch_decode_windows_dense on the GPU (include/acm_hip.h; libacm_amd/csrc/acm_batch_windows.cpp, acm_dense.hip): the windows of a
call as the rows of one tensor.

Every call writes into a buffer of its own, poisoned, with one guard row in front of the tensor and one behind it: the tensor then starts
at every alignment a row length allows, the guards must keep the poison and the rows must be the expected ones exactly - zeros behind a
window's samples, so no poison inside either.  The handle's fill mode is on (helpers): the intermediate PCM arena starts every call at
0xA5, and a gather that reads a place the synthesis did not write shows up as 0xA5A5, not as the previous call's samples.

Expected rows: tests/dense_crops.py (the oracle's whole-file decode and the contract's formula; tests/test_dense_crops.py holds the case
list to what it has to reach).  Nothing here existed at the parent commit: the symbol is new."""
import numpy as np
import pytest

import dense_crops as DC
from helpers import make_stream
from libacm_amd import capi

pytestmark = pytest.mark.gpu

POISON = 0xC7                   # not the arenas' 0xA5, not zero, and 0xC7C7C7C7 is no float the kernel can make of an int16
BOTH = (capi.PARSE_HOST, capi.PARSE_DEVICE)


def run(dev, files, index, windows, frames, channels, planar, f32, parse, check=True, threads=4, **kw):
    """one call into the middle of a poisoned buffer of N + 2 rows -> (the N rows as written, statuses, words, timing[, rc]); the guard
    rows must come back as poison"""
    n, R = len(windows), frames * channels
    unit, dt = (4, np.uint32) if f32 else (2, np.uint16)
    total = (n + 2) * R
    d = dev.malloc(total * unit)
    try:
        dev.memset(d, POISON, total * unit)
        res = capi.batch_decode_windows_dense(dev, files, index, windows, d + R * unit, n * R, frames, channels=channels, planar=planar, f32=f32,
                                              parse=parse, threads=threads, check=check, **kw)
        raw = np.zeros(total, dtype=dt)
        dev.download(raw, d)
    finally:
        dev.free(d)
    poison = np.frombuffer(bytes([POISON]) * unit, dtype=dt)[0]
    assert (raw[:R] == poison).all(), "the call wrote in front of its tensor"
    assert (raw[total - R:] == poison).all(), "the call wrote behind its tensor"
    return (raw[R:total - R].reshape(n, R),) + tuple(res)


def same(got, want_i16, f32):
    """bit for bit: int16 rows, or float32 rows that are the int16 ones times 2^-15 (a padded element is +0.0)"""
    if f32:
        return np.array_equal(got, DC.as_f32(want_i16).view(np.uint32))
    return np.array_equal(got, want_i16.view(np.uint16))


def data_and_index():
    return [f.data for f in DC.files()], DC.index_of()


def deinterleave(row_i16, frames, channels):
    return np.ascontiguousarray(row_i16.reshape(frames, channels).T).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- expected rows

@pytest.mark.parametrize("parse", BOTH, ids=["host", "device"])
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("case", DC.cases(), ids=lambda c: c.name)
def test_expected_rows(dev, case, f32, planar, parse):
    files, index = data_and_index()
    got, st, words, tm = run(dev, files, index, case.windows, case.frames, case.channels, planar, f32, parse)
    want = case.rows(planar)
    nblocks = 0
    for k in range(len(case.windows)):
        w, status, nb = case.expect(k)
        nblocks += nb
        assert (words[k], st[k]) == (w, status), (k, case.windows[k], words[k], st[k], w, status)
        assert same(got[k], want[k], f32), "row %d, window %r: %d of %d elements differ, the first at %d" % (
            k, case.windows[k], int((got[k] != (DC.as_f32(want[k]).view(np.uint32) if f32 else want[k].view(np.uint16))).sum()), case.row,
            int(np.nonzero(got[k] != (DC.as_f32(want[k]).view(np.uint32) if f32 else want[k].view(np.uint16)))[0][0]))
    assert tm.blocks_parsed == nblocks and tm.samples == sum(words)
    assert (tm.device_parsed > 0) == (parse == capi.PARSE_DEVICE)


# ---------------------------------------------------------------------------------------------------------------- the windows call

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("case", DC.cases(), ids=lambda c: c.name)
def test_agrees_with_the_windows_call(dev, case, f32):
    """words and status are acm_batch_decode_windows' for the same window, and the head of the row is that call's window - whatever the
    oracle says"""
    files, index = data_and_index()
    keep = [k for k in range(len(case.windows)) if not case.rejected(k)]            # (the windows call knows no channel count)
    wins = [case.windows[k] for k in keep]
    cap = capi.batch_window_pcm_words(files, wins)
    unit, dt = (4, np.uint32) if f32 else (2, np.uint16)
    for parse in BOTH:
        d = dev.malloc(max(cap, 1) * unit)
        try:
            w_st, w_words, w_offs, _, w_tm = capi.batch_decode_windows_device(dev, files, index, wins, d, cap, parse=parse, f32=f32, threads=4)
            flat = np.zeros(max(cap, 1), dtype=dt)
            dev.download(flat, d)
        finally:
            dev.free(d)
        for planar in (False, True):
            got, st, words, tm = run(dev, files, index, wins, case.frames, case.channels, planar, f32, parse)
            assert st == w_st and words == w_words and tm.blocks_parsed == w_tm.blocks_parsed
            for k in range(len(wins)):
                win = np.zeros(case.row, dtype=dt)
                win[:words[k]] = flat[w_offs[k]:w_offs[k] + words[k]]
                if planar:
                    win = deinterleave(win, case.frames, case.channels)
                assert np.array_equal(got[k], win), (k, wins[k], planar, parse)


# ---------------------------------------------------------------------------------------------------------------- turned away during the call

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
def test_a_window_the_stager_rejects_is_a_row_of_zeros(dev, f32):
    """the marks of another file of the same shape: the index passes the checks in front of the call, the stager (or the device walk and
    then the stager) finds blocks that are not where it says.  Those windows get the windows call's status and a row of zeros; the other
    file's rows between them are whole"""
    a, b = make_stream(9300, 7, 16, 12, mix=1), make_stream(9301, 7, 16, 12, mix=1)
    fa, fb = DC.File(a), DC.File(b)
    n = int((fb.marks["bit"][:fa.marks.size] <= 8 * len(a)).sum())          # as much of the foreign index as the file could have
    assert n >= 10
    stale = [fb.marks[:n].copy(), fb.marks]
    bl, T = fa.st.block_len, 48
    windows = [(1, 5, T), (0, 3 * bl + 11, T), (1, 2 * bl + 5, 40), (0, 0, T), (0, 7 * bl - 9, 33), (1, bl - 7, T), (0, 5 * bl + 1, 1), (1, 77, T)]
    for parse in BOTH:
        cap = capi.batch_window_pcm_words([a, b], windows)
        d = dev.malloc(cap * 2)
        try:
            w_st, w_words = capi.batch_decode_windows_device(dev, [a, b], stale, windows, d, cap, parse=parse, threads=4)[:2]
        finally:
            dev.free(d)
        turned_away = [k for k, s in enumerate(w_st) if s != 0 and w_words[k] == 0]
        assert turned_away and all(w_st[k] == 0 for k, w in enumerate(windows) if w[0] == 1)
        for planar in (False, True):
            got, st, words, tm = run(dev, [a, b], stale, windows, T, 1, planar, f32, parse)
            assert st == w_st and words == w_words
            for k, (f, first, count) in enumerate(windows):
                want = np.zeros(T, np.int16)
                want[:words[k]] = (fa, fb)[f].pcm[first:first + words[k]]          # a window the stager let through is the file's own PCM
                assert words[k] == count or st[k] != 0
                assert same(got[k], want, f32), (k, windows[k], parse)
        # the same handle, the right index: every row whole
        got, st, words, tm = run(dev, [a, b], [fa.marks, fb.marks], windows, T, 1, False, f32, parse)
        assert st == [0] * len(windows) and all(same(got[k, :c], (fa, fb)[f].pcm[s:s + c], f32) for k, (f, s, c) in enumerate(windows))


def test_another_channel_count_is_turned_away_before_anything_is_parsed(dev):
    files, index = data_and_index()
    mono = [(0, 8, 64), (2, 100, 40), (4, 510, 64), (2, 4, 2)]
    stereo = [(1, 8, 64), (5, 1000, 32), (3, 0, 0)]
    for parse in BOTH:
        alone, st0, words0, tm0 = run(dev, files, index, mono, 64, 1, True, False, parse)
        mixed = [mono[0], stereo[0], mono[1], stereo[1], stereo[2], mono[2], mono[3]]
        got, st, words, tm = run(dev, files, index, mixed, 64, 1, True, False, parse)
        assert [st[k] for k in (1, 3, 4)] == [capi.ERR_ARG] * 3 and [words[k] for k in (1, 3, 4)] == [0, 0, 0]
        assert not got[[1, 3, 4]].any()
        assert np.array_equal(got[[0, 2, 5, 6]], alone) and [st[k] for k in (0, 2, 5, 6)] == st0 == [0] * 4
        assert tm.blocks_parsed == tm0.blocks_parsed > 0 and tm.samples == tm0.samples and tm.h2d_bytes == tm0.h2d_bytes + 16 * 3
        # and the other way round: a stereo batch turns the mono files away
        got, st, words, tm = run(dev, files, index, mixed, 32, 2, True, False, parse)
        assert [st[k] for k in (0, 2, 5, 6)] == [capi.ERR_ARG] * 4 and not got[[0, 2, 5, 6]].any() and st[1] == st[3] == st[4] == 0
        assert np.array_equal(got[1].view(np.int16), deinterleave(DC.files()[1].pcm[8:72], 32, 2))


# ---------------------------------------------------------------------------------------------------------------- many rows

def test_66000_rows(dev):
    """more rows than any 16-bit grid dimension holds, 8 stereo frames each, split into planes and widened: a seeded sample of 500 rows,
    the first and the last.  75 000 windows: one in nine is empty and an empty window gets no parse job (acm_window_layout.cpp), so
    only from about 73 800 windows on do more than 65 535 of them reach the device parser, whose column kernel then walks its job
    table in a second slice (acm_parse.hip: launch_columns, d_jobs + at)"""
    files, index = data_and_index()
    rng = np.random.default_rng(66000)
    n, T = 75000, 8
    src = rng.choice([1, 3], n)
    first = 2 * (rng.integers(0, 1 << 30, n) % np.array([(DC.files()[f].words - 2) // 2 for f in src]))
    count = 2 * rng.integers(0, T + 1, n)
    windows = list(zip(src.tolist(), first.tolist(), count.tolist()))
    got, st, words, tm = run(dev, files, index, windows, T, 2, True, True, capi.PARSE_AUTO, threads=0)
    assert tm.device_parsed > 65535
    delivering = [k for k, w in enumerate(words) if w]
    assert len(delivering) > 65535
    for k in [0, n - 1, delivering[65534], delivering[65535], delivering[-1]] + rng.choice(n, 500, replace=False).tolist():
        f, a, c = windows[k]
        w = max(0, min(c, DC.files()[f].words - a))
        want = np.zeros(2 * T, np.int16)
        want[:w] = DC.files()[f].pcm[a:a + w]
        assert words[k] == w and same(got[k], deinterleave(want, T, 2), True), (k, windows[k])


# ---------------------------------------------------------------------------------------------------------------- python

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
def test_gpu_decoder_crop_batch(f32):
    import torch
    from libacm_amd import batch
    fs = DC.files()
    files = [fs[k].data for k in (1, 3, 5, 7, 0)]
    dec = batch.GpuDecoder(0, parse=capi.PARSE_DEVICE, dtype=torch.float32 if f32 else torch.int16)
    try:
        index = batch.build_index(files, threads=2)
        T = 50
        windows = [(0, 0, T), (1, 37, T), (2, 300, 41), (1, fs[3].words // 2 - 10, T), (3, 0, 5), (4, 3, 20), (2, 511, 1), (0, 9, 0)]
        flat, offs, counts, sts = dec.crop(files, [(f, 2 * a, 2 * c) for f, a, c in windows], index)
        flat = flat.cpu().numpy()
        for planar in (True, False):
            batch_t, frames, st = dec.crop_batch(files, windows, T, channels=2, planar=planar, index=index)
            assert batch_t.dtype == dec.dtype and batch_t.is_cuda and tuple(batch_t.shape) == ((8, 2, T) if planar else (8, T, 2))
            got = batch_t.cpu().numpy()
            for k, (f, a, c) in enumerate(windows):
                if f == 4:
                    assert st[k] == capi.ERR_ARG and frames[k] == 0 and not got[k].any()
                    continue
                assert st[k] == sts[k] and 2 * frames[k] == counts[k]
                want = np.zeros((T, 2), got.dtype)
                want[:frames[k]] = flat[offs[k]:offs[k] + counts[k]].reshape(-1, 2)
                assert np.array_equal(got[k].view(np.uint8), np.ascontiguousarray(want.T if planar else want).view(np.uint8)), (k, planar)
        # out=: a buffer large enough is written into and the batch is a view of it; one that is too small, or of the other dtype, is not
        out = torch.full((8 * 2 * T + 100,), 77, dtype=dec.dtype, device="cuda:0")
        batch_t, frames, st = dec.crop_batch(files, windows, T, channels=2, planar=True, index=index, out=out)
        assert batch_t.data_ptr() == out.data_ptr() and np.array_equal(batch_t.cpu().numpy().view(np.uint8), got.transpose(0, 2, 1).copy().view(np.uint8))
        assert (out[8 * 2 * T:] == 77).all()
        small = torch.empty(8 * 2 * T - 1, dtype=dec.dtype, device="cuda:0")
        batch_t, frames, st = dec.crop_batch(files, windows, T, channels=2, index=index, out=small)
        assert batch_t.data_ptr() != small.data_ptr() and tuple(batch_t.shape) == (8, 2, T)
        with pytest.raises(ValueError):
            dec.crop_batch(files, windows, T, channels=2, index=index, out=torch.empty(8 * 2 * T, dtype=torch.int32, device="cuda:0"))
        # mono, the index built by the call itself
        batch_t, frames, st = dec.crop_batch(files, [(4, 10, 30), (4, 600, 30)], 32)
        assert tuple(batch_t.shape) == (2, 1, 32) and frames == [30, 30] and st == [0, 0]
    finally:
        dec.dev.close()


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_refused_calls_write_nothing(dev):
    files, index = data_and_index()
    wins, T = [(0, 8, 32), (2, 16, 64)], 64

    def refused(what, windows=wins, frames=T, channels=1, want=capi.ERR_ARG, **kw):
        n, R = len(windows), (frames or 1) * (channels if channels in (1, 2) else 1)
        d = dev.malloc((n + 2) * R * 2)
        try:
            dev.memset(d, POISON, (n + 2) * R * 2)
            kw.setdefault("d_pcm", d + 2 * R)
            kw.setdefault("d_pcm_words", n * R)
            res = capi.batch_decode_windows_dense(kw.pop("device", dev), files, index, windows, kw.pop("d_pcm"), kw.pop("d_pcm_words"), frames, channels=channels,
                                                  check=False, threads=2, **kw)
            raw = np.zeros((n + 2) * R, np.uint16)
            dev.download(raw, d)
        finally:
            dev.free(d)
        assert res[-1] == want, (what, res[-1])
        assert (raw == POISON * 0x101).all(), what

    refused("no acm_dense_opts", frames=None)
    refused("frames == 0", frames=0)
    refused("channels == 0", channels=0)
    refused("channels == 3", channels=3)
    refused("unknown dense flag", dense_flags=2)
    refused("no output", d_pcm=None)
    refused("output one sample short", d_pcm_words=2 * T - 1)
    for fmt in (capi.FMT_S16BE, capi.FMT_U16LE, capi.FMT_U16BE):
        refused("fmt %d" % fmt, fmt=fmt)
    refused("packed staging", batch_flags=capi.BATCH_STAGE_PACKED)
    refused("max_words > R", windows=wins + [(0, 0, T + 1)])
    refused("odd first_word", windows=[(1, 3, 8)] + wins, channels=2)
    refused("odd max_words", windows=wins + [(1, 4, 7)], channels=2)
    refused("no device", device=None, want=capi.ERR_NO_DEVICE)
    # prestaged: any non-null pointer is refused before it is looked at
    L = capi.lib()
    import ctypes as C
    bufs, items, ix, w, keep = capi._window_tables(files, index, wins)
    d = dev.malloc(4 * T * 2)
    try:
        dev.memset(d, POISON, 4 * T * 2)
        opts = capi.BatchOpts(0, 0, 2, 0, capi.PARSE_HOST, 0, d + 2 * T, 2 * T, 0x1000)
        dense = capi.DenseOpts(T, 1, 0)
        assert L.acm_batch_decode_windows_dense(dev.h, items, len(files), ix, w, 2, C.byref(opts), C.byref(dense), None) == capi.ERR_ARG
        raw = np.zeros(4 * T, np.uint16)
        dev.download(raw, d)
        assert (raw == POISON * 0x101).all()
        # ... and the accepted call next to them all: the same arguments without the fault, no timing asked for
        opts.prestaged = None
        assert L.acm_batch_decode_windows_dense(dev.h, items, len(files), ix, w, 2, C.byref(opts), C.byref(dense), None) == 0
        dev.download(raw, d)
    finally:
        dev.free(d)
    assert (raw[:T] == POISON * 0x101).all() and (raw[3 * T:] == POISON * 0x101).all()
    assert np.array_equal(raw[T:T + 32].view(np.int16), DC.files()[0].pcm[8:40]) and not raw[T + 32:2 * T].any()
    assert np.array_equal(raw[2 * T:3 * T].view(np.int16), DC.files()[2].pcm[16:80])
