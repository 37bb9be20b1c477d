"""acm_batch_decode_windows_dense with ACM_DENSE_SPEED on the GPU (include/acm_hip.h; libacm_amd/csrc/acm_batch_windows.cpp,
acm_dense_speed.hip): a speed per window, and ratios whose exact table would not fit, as rows of one tensor.

Every call writes into the middle of a poisoned buffer with a guard row on either side: the guards must keep the poison and the rows
must be the model's exactly - both filters are defined on integers, so there is no tolerance.  The handle's fill mode is on (helpers): a
kernel that reads a place the synthesis did not write shows up as 0xA5A5.

Expected rows: tests/dense_speed.py (the oracle's whole-file decode, the channel conversion, then the contract's classification and
filter with the library's own tables; tests/test_dense_speed.py holds the tables to the contract and the case list to what it has to
reach).  Every call here sets dense flag 32, which the library refused before it knew ACM_DENSE_SPEED."""
import numpy as np
import pytest

import dense_crops as DC
import dense_resample as DR
import dense_speed as DS
import helpers  # noqa: F401  (the fill mode of the handle, as in every module of GPU tests)
from libacm_amd import capi
from test_gpu_dense_crops import BOTH, POISON, same

pytestmark = pytest.mark.gpu

_plain = {}


def data_and_index():
    return [f.data for f in DR.files()], DC.index_of(DR.files())


def run(dev, windows, speeds, frames, channels, planar, f32, parse, rate, mix, shift=0, check=True, **kw):
    """one call with the speeds into a poisoned buffer: a guard row, `shift` elements, the N rows, a guard row -> (the N rows as
    written, statuses, words, timing[, rc]); everything around the rows must come back as poison"""
    files, index = data_and_index()
    n, R = len(windows), frames * channels
    unit, dt = (4, np.uint32) if f32 else (2, np.uint16)
    total = (n + 2) * R + shift
    d = dev.malloc(total * unit)
    try:
        assert d % 256 == 0
        dev.memset(d, POISON, total * unit)
        res = capi.batch_decode_windows_dense(dev, files, index, windows, d + (R + shift) * unit, n * R, frames, channels=channels, planar=planar,
                                              f32=f32, parse=parse, threads=4, mix=mix, rate=rate, speeds=speeds, check=check, **kw)
        raw = np.zeros(total, dtype=dt)
        dev.download(raw, d)
    finally:
        dev.free(d)
    poison = np.frombuffer(bytes([POISON]) * unit, dtype=dt)[0]
    assert (raw[:R + shift] == poison).all(), "the call wrote in front of its tensor"
    assert (raw[total - R:] == poison).all(), "the call wrote behind its tensor"
    return (raw[R + shift:total - R].reshape(n, R),) + tuple(res)


def windows_call(dev, case, parse):
    """(kept windows, statuses, words, blocks_parsed) of acm_batch_decode_windows for the case's windows that are not turned away: once
    per case and parser"""
    key = (case.name, parse)
    if key not in _plain:
        files, index = data_and_index()
        keep = [k for k, w in enumerate(case.windows) if w[0] >= len(DR.files()) or case.filter(k) is not None]
        wins = [case.windows[k] for k in keep]
        cap = capi.batch_window_pcm_words(files, wins)
        d = dev.malloc(max(cap, 1) * 2)
        try:
            st, words, _, _, tm = capi.batch_decode_windows_device(dev, files, index, wins, d, cap, parse=parse, threads=4)
        finally:
            dev.free(d)
        _plain[key] = (keep, st, words, tm.blocks_parsed)
    return _plain[key]


def check_rows(case, got, st, words, planar, f32):
    want = case.rows(planar)
    nblocks = 0
    for k in range(len(case.windows)):
        w, status, nb = case.expect(k)
        nblocks += nb
        assert (words[k], st[k]) == (w, status), (k, case.windows[k], words[k], st[k], w, status)
        if not same(got[k], want[k], f32):
            ref = DC.as_f32(want[k]).view(np.uint32) if f32 else want[k].view(np.uint16)
            bad = np.nonzero(got[k] != ref)[0]
            flt = case.filter(k)
            raise AssertionError("row %d, window %r at speed %r (%s): %d of %d elements differ, the first at %d" % (
                k, case.windows[k], case.speeds[k], flt.kind if flt else "turned away", bad.size, got[k].size, int(bad[0])))
    return nblocks


# ---------------------------------------------------------------------------------------------------------------- expected rows

@pytest.mark.parametrize("parse", BOTH, ids=["host", "device"])
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("case", DS.cases(), ids=lambda c: c.name)
def test_expected_rows(dev, case, f32, planar, parse):
    got, st, words, tm = run(dev, case.windows, case.speeds, case.frames, case.channels, planar, f32, parse, case.rate, case.mix)
    nblocks = check_rows(case, got, st, words, planar, f32)
    assert tm.blocks_parsed == nblocks and tm.samples == sum(words)
    assert (tm.device_parsed > 0) == (parse == capi.PARSE_DEVICE)
    # words and status are the windows call's for the same windows, and so are the blocks parsed
    keep, w_st, w_words, w_blocks = windows_call(dev, case, parse)
    assert [st[k] for k in keep] == w_st and [words[k] for k in keep] == w_words and tm.blocks_parsed == w_blocks
    assert all(st[k] == capi.ERR_ARG and words[k] == 0 and not got[k].any() for k in set(range(len(st))) - set(keep))


# ---------------------------------------------------------------------------------------------------------------- an odd element offset

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("case", [c for c in DS.cases() if c.mix and c.frames in (37, 2100, DS.STEEP_T)], ids=lambda c: c.name)
def test_tensor_one_element_off_a_line(dev, case, f32):
    """the tensor begins one element behind a 16-byte line: every row has single outputs in front of its first line, and the vectors
    of an interleaved stereo row begin on a frame's second channel"""
    got, st, words, tm = run(dev, case.windows, case.speeds, case.frames, case.channels, False, f32, capi.PARSE_DEVICE, case.rate, True, shift=1)
    check_rows(case, got, st, words, False, f32)


# ---------------------------------------------------------------------------------------------------------------- the flag alone

@pytest.mark.parametrize("case", [c for c in DR.cases() if c.frames != 64], ids=lambda c: c.name)
def test_all_speeds_zero_is_the_call_without_the_flag(dev, case):
    """tests/dense_resample.py's cases with flag 32 and every speed 0: the tensor of the call without the flag, byte for byte, and as
    many bytes sent - the same kernel over the same tables.  (Without the file at 22051 Hz: the flag is what takes its windows)"""
    windows = [w for w in case.windows if w[0] != 8]
    want = {planar: case.rows(planar)[[k for k, w in enumerate(case.windows) if w[0] != 8]] for planar in (False, True)}
    for f32, planar, parse in ((False, False, capi.PARSE_HOST), (True, True, capi.PARSE_DEVICE)):
        plain, st0, words0, tm0 = run(dev, windows, None, case.frames, case.channels, planar, f32, parse, DR.RATE, case.mix)
        zeros, st1, words1, tm1 = run(dev, windows, [None] * len(windows), case.frames, case.channels, planar, f32, parse, DR.RATE, case.mix)
        ones, st2, words2, tm2 = run(dev, windows, [(1, 1)] * len(windows), case.frames, case.channels, planar, f32, parse, DR.RATE, case.mix)
        assert plain.any() and plain.tobytes() == zeros.tobytes() == ones.tobytes()
        assert st0 == st1 == st2 and words0 == words1 == words2
        assert (tm0.blocks_parsed, tm0.samples, tm0.h2d_bytes) == (tm1.blocks_parsed, tm1.samples, tm1.h2d_bytes) == (tm2.blocks_parsed, tm2.samples, tm2.h2d_bytes)
        assert same(plain, want[planar], f32)


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_refused_calls_write_nothing(dev):
    wins, T = [(2, 8, 32), (4, 16, 128), (0, 4, 32)], 64
    sp = [(9, 10), None, (1001, 1000)]
    RS, SP = capi.DENSE_RESAMPLE, capi.DENSE_SPEED
    for what, windows, speeds, kw in (
            ("the flag without ACM_DENSE_RESAMPLE", wins, sp, dict(dense_flags=SP)),
            ("a speed with no denominator", wins, [(9, 0), None, None], {}),
            ("a speed with no numerator", wins, [None, None, (0, 7)], {}),
            ("a window one frame too long at 9/10", wins + [(2, 0, 58)], sp + [(9, 10)], {}),
            ("a window one frame too long at 29999/30000", wins + [(2, 0, 64)], sp + [DS.NEAR_ONE], {})):
        got, st, words, tm, rc = run(dev, windows, speeds, T, 1, False, False, capi.PARSE_HOST, DR.RATE, False, check=False, **kw)
        assert rc == capi.ERR_ARG, (what, rc)
        assert (got == POISON * 0x101).all(), what
    # the accepted calls next to them: the longest windows
    for windows, speeds in ((wins + [(2, 0, 57)], sp + [(9, 10)]), (wins + [(2, 0, 63)], sp + [DS.NEAR_ONE])):
        got, st, words, tm, rc = run(dev, windows, speeds, T, 1, False, False, capi.PARSE_HOST, DR.RATE, False, check=False)
        assert rc == 0 and st == [0] * 4 and words == [w[2] for w in windows]
        for k, (w, s) in enumerate(zip(windows, speeds)):
            assert np.array_equal(got[k].view(np.int16), DS.row_of(*w, s, 1, T, False, False, DR.RATE)), k
    assert DS.Filter(22050, 22050, (9, 10)).n_out(57) == 64 and DS.Filter(22050, 22050, DS.NEAR_ONE).n_out(63) == 64


# ---------------------------------------------------------------------------------------------------------------- python

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
def test_gpu_decoder_crop_batch_speed(f32):
    """windows in frames over the files, three speeds a file, whatever their channel count and rate"""
    import torch
    from libacm_amd import batch
    fs = DR.files()
    files = [f.data for f in fs]
    dec = batch.GpuDecoder(0, parse=capi.PARSE_DEVICE, dtype=torch.float32 if f32 else torch.int16)
    try:
        index = batch.build_index(files, threads=2)
        T = 50
        assert [batch.source_frames(T, 22050, DR.RATE, s) for s in ((9, 10), (1, 1), (11, 10))] == [45, 50, 55]
        assert batch.source_frames(T, 22050, 16000, (9, 10)) == 62 and batch.source_frames(T, 22051, DR.RATE) == 50
        windows, speed = [], []
        for f in (0, 3, 5, 6, 8, 10):
            for s in ((9, 10), None, (11, 10)):
                # (a file without a rate is checked as a row of the batch's own at speed 1: T frames at most)
                windows.append((f, 11 + f, batch.source_frames(T, DR.rate_of(f), DR.RATE, s or (1, 1)) if DR.rate_of(f) else T))
                speed.append(s)
        for channels, planar in ((1, True), (2, True), (2, False)):
            batch_t, frames, st = dec.crop_batch(files, windows, T, channels=channels, planar=planar, index=index, mix=True, rate=DR.RATE, speed=speed)
            n = len(windows)
            assert batch_t.dtype == dec.dtype and batch_t.is_cuda and tuple(batch_t.shape) == ((n, channels, T) if planar else (n, T, channels))
            got = batch_t.cpu().numpy().reshape(n, -1)
            for k, ((f, a, m), s) in enumerate(zip(windows, speed)):
                c = DR.chans_of(f, channels)
                want = DS.row_of(f, a * c, m * c, s, channels, T, planar, True, DR.RATE)
                assert np.array_equal(got[k].view(np.uint8), (DC.as_f32(want) if f32 else want).view(np.uint8)), (k, channels, planar)
                assert frames[k] == (0 if f == 10 else DS.filter_of(f, DR.RATE, s)[0].n_out(m)) <= T, (k, frames[k])
        with pytest.raises(ValueError):
            dec.crop_batch(files, windows, T, index=index, speed=speed)
    finally:
        dec.dev.close()
