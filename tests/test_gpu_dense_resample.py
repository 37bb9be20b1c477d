"""acm_batch_decode_windows_dense with ACM_DENSE_RESAMPLE on the GPU (include/acm_hip.h; libacm_amd/csrc/acm_batch_windows.cpp,
acm_dense_resample.hip): files of several sample rates as the rows of one tensor at one rate.

Every call writes into the middle of a poisoned buffer with a guard row on either side (tests/test_gpu_dense_crops.py::run): the guards
must keep the poison and the rows must be the model's exactly - the filter is defined on integers, so there is no tolerance.  The
handle's fill mode is on (helpers): a kernel that reads a place the synthesis did not write shows up as 0xA5A5.

Expected rows: tests/dense_resample.py (the oracle's whole-file decode, the channel conversion, then the contract's filter with the
library's own taps; tests/test_dense_resample.py holds the taps to the contract and the case list to what it has to reach).  Every call
here sets dense flag 16, which the library refused before it knew ACM_DENSE_RESAMPLE."""
import numpy as np
import pytest

import dense_crops as DC
import dense_resample as DR
import helpers  # noqa: F401  (the fill mode of the handle, as in every module of GPU tests)
from libacm_amd import capi
from test_gpu_dense_crops import BOTH, POISON, run, same

pytestmark = pytest.mark.gpu

_plain = {}


def data_and_index():
    return [f.data for f in DR.files()], DC.index_of(DR.files())


def windows_call(dev, case, parse):
    """(statuses, words, blocks_parsed) of acm_batch_decode_windows for the case's windows that are not turned away: once per case
    and parser"""
    key = (case.name, parse)
    if key not in _plain:
        files, index = data_and_index()
        keep = [k for k, w in enumerate(case.windows) if w[0] >= len(DR.files()) or not DR.turned_away(w[0], case.channels, case.mix)]
        wins = [case.windows[k] for k in keep]
        cap = capi.batch_window_pcm_words(files, wins)
        d = dev.malloc(max(cap, 1) * 2)
        try:
            st, words, _, _, tm = capi.batch_decode_windows_device(dev, files, index, wins, d, cap, parse=parse, threads=4)
        finally:
            dev.free(d)
        _plain[key] = (keep, st, words, tm.blocks_parsed)
    return _plain[key]


def first_difference(got, want_i16, f32):
    want = DC.as_f32(want_i16).view(np.uint32) if f32 else want_i16.view(np.uint16)
    bad = np.nonzero(got != want)[0]
    return "%d of %d elements differ, the first at %d" % (bad.size, got.size, int(bad[0]))


def check_rows(case, got, st, words, planar, f32):
    want = case.rows(planar)
    nblocks = 0
    for k in range(len(case.windows)):
        w, status, nb = case.expect(k)
        nblocks += nb
        assert (words[k], st[k]) == (w, status), (k, case.windows[k], words[k], st[k], w, status)
        assert same(got[k], want[k], f32), "row %d, window %r, filtered %d: %s" % (k, case.windows[k], case.filtered(k),
                                                                                  first_difference(got[k], want[k], f32))
    return nblocks


# ---------------------------------------------------------------------------------------------------------------- expected rows

@pytest.mark.parametrize("parse", BOTH, ids=["host", "device"])
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("case", DR.cases(), ids=lambda c: c.name)
def test_expected_rows(dev, case, f32, planar, parse):
    files, index = data_and_index()
    got, st, words, tm = run(dev, files, index, case.windows, case.frames, case.channels, planar, f32, parse, mix=case.mix, rate=DR.RATE)
    nblocks = check_rows(case, got, st, words, planar, f32)
    assert tm.blocks_parsed == nblocks and tm.samples == sum(words)
    assert (tm.device_parsed > 0) == (parse == capi.PARSE_DEVICE)
    # words and status are the windows call's for the same windows, and so are the blocks parsed
    keep, w_st, w_words, w_blocks = windows_call(dev, case, parse)
    assert [st[k] for k in keep] == w_st and [words[k] for k in keep] == w_words and tm.blocks_parsed == w_blocks
    assert all(st[k] == capi.ERR_ARG and words[k] == 0 and not got[k].any() for k in set(range(len(st))) - set(keep))


# ---------------------------------------------------------------------------------------------------------------- an odd element offset

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("case", [c for c in DR.cases() if c.mix and c.frames != 64], ids=lambda c: c.name)
def test_tensor_one_element_off_a_line(dev, case, f32):
    """the tensor begins one element behind a 16-byte line: every row has single outputs in front of its first line, and the vectors
    of an interleaved stereo row begin on a frame's second channel.  Guards: the element in front of the tensor, a row in front of that
    and a row behind"""
    files, index = data_and_index()
    n, R = len(case.windows), case.row
    unit, dt = (4, np.uint32) if f32 else (2, np.uint16)
    total = (n + 2) * R + 1
    d = dev.malloc(total * unit)
    try:
        assert d % 256 == 0
        dev.memset(d, POISON, total * unit)
        st, words, tm = capi.batch_decode_windows_dense(dev, files, index, case.windows, d + (R + 1) * unit, n * R, case.frames, channels=case.channels,
                                                        planar=False, f32=f32, parse=capi.PARSE_DEVICE, threads=4, mix=True, rate=DR.RATE)
        raw = np.zeros(total, dtype=dt)
        dev.download(raw, d)
    finally:
        dev.free(d)
    poison = np.frombuffer(bytes([POISON]) * unit, dtype=dt)[0]
    assert (raw[:R + 1] == poison).all(), "the call wrote in front of its tensor"
    assert (raw[total - R:] == poison).all(), "the call wrote behind its tensor"
    check_rows(case, raw[R + 1:total - R].reshape(n, R), st, words, False, f32)


# ---------------------------------------------------------------------------------------------------------------- the steepest ratio

@pytest.mark.parametrize("channels,planar,f32", [(1, False, False), (2, False, True), (2, True, False), (1, False, True)],
                         ids=["mono", "interleaved_f32", "planar", "mono_f32"])
def test_down_by_eight_takes_two_passes(dev, channels, planar, f32):
    """16000 -> 2000 Hz: M = 8 L and K = 128, the most source a unit of outputs can need - more than the kernel's planes hold, so a
    unit is worked off in two passes of 1024 outputs, each staging its own span; T = 1100 has outputs on either side of the seam.
    11025 -> 2000 (L = 80, M = 441, K = 90) beside it in one pass; 22050 and 44100 Hz are no ratios the filter takes"""
    files, index = data_and_index()
    rate, T = 2000, 1100
    assert DR.ratio(16000, rate) == (1, 8, 128, 64) and DR.ratio(11025, rate) == (80, 441, 90, 45) and DR.ratio(22050, rate) is None
    wins = [(6, 3, 8800), (2, 8, 64), (0, 5, 6063), (6, 1000, 8799), (7, 2, 10000), (4, 0, 8), (6, 16, 8193), (1, 6, 2 * 4000), (6, 40, 63), (7, 8, 2 * 4100)]
    got, st, words, tm = run(dev, files, index, wins, T, channels, planar, f32, capi.PARSE_DEVICE, mix=True, rate=rate)
    for k, (f, first, count) in enumerate(wins):
        bad = f in (2, 4)
        assert (words[k], st[k]) == ((0, capi.ERR_ARG) if bad else (count, 0)), (k, wins[k])
        want = DR.row_of(f, first, count, channels, T, planar, True, rate=rate)
        assert want.any() != bad and same(got[k], want, f32), "row %d, window %r: %s" % (k, wins[k], first_difference(got[k], want, f32))
    assert DR.frames_out(6, 3, 8800, channels, True, rate) == T and DR.frames_out(6, 16, 8193, channels, True, rate) == 1025


# ---------------------------------------------------------------------------------------------------------------- the flag alone

def test_the_flag_over_one_rate_changes_nothing(dev):
    """a batch whose files are all at the batch's rate, with the flag set: bit for bit the call without it, and as many bytes sent"""
    files, index = data_and_index()
    for C, own in ((1, 2), (2, 3)):
        W = DR.files()[own].words
        wins = [(own, 8 * C, 64 * C), (own, 3 * C, 5 * C), (10, 0, 0), (own, W - 6 * C, 64 * C), (own, 40 * C, 63 * C), (99, 0, 2 * C)]
        for f32, planar, parse in ((False, False, capi.PARSE_HOST), (True, True, capi.PARSE_DEVICE)):
            plain, st0, words0, tm0 = run(dev, files, index, wins, 64, C, planar, f32, parse)
            flagged, st1, words1, tm1 = run(dev, files, index, wins, 64, C, planar, f32, parse, rate=DR.RATE)
            assert np.array_equal(plain, flagged) and plain.any()
            assert st0 == st1 and words0 == words1 and (tm0.blocks_parsed, tm0.samples, tm0.h2d_bytes) == (tm1.blocks_parsed, tm1.samples, tm1.h2d_bytes)


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_refused_calls_write_nothing(dev):
    files, index = data_and_index()
    wins, T = [(2, 8, 32), (4, 16, 128), (0, 4, 32)], 64

    def call(windows, **kw):
        n = len(windows)
        d = dev.malloc((n + 2) * T * 2)
        try:
            dev.memset(d, POISON, (n + 2) * T * 2)
            res = capi.batch_decode_windows_dense(dev, files, index, windows, d + 2 * T, n * T, T, channels=1, check=False, threads=2, **kw)
            raw = np.zeros((n + 2) * T, np.uint16)
            dev.download(raw, d)
        finally:
            dev.free(d)
        return res, raw

    for what, windows, kw in (("rate == 0", wins, dict(dense_flags=capi.DENSE_RESAMPLE)),
                              ("a 44100 Hz window one frame too long", wins + [(4, 0, 130)], dict(rate=DR.RATE)),
                              ("an 11025 Hz window one frame too long", wins + [(0, 0, 33)], dict(rate=DR.RATE)),
                              ("odd first_word on a stereo item", wins + [(5, 3, 8)], dict(rate=DR.RATE, mix=True)),
                              ("odd max_words on a stereo item", wins + [(5, 4, 7)], dict(rate=DR.RATE, mix=True))):
        res, raw = call(windows, **kw)
        assert res[-1] == capi.ERR_ARG, (what, res[-1])
        assert (raw == POISON * 0x101).all(), what
    # the accepted call next to them: the longest windows of either ratio
    res, raw = call(wins, rate=DR.RATE)
    assert res[-1] == 0 and res[0] == [0, 0, 0] and res[1] == [32, 128, 32]
    assert all(np.array_equal(raw[(k + 1) * T:(k + 2) * T].view(np.int16), DR.row_of(*w, 1, T, False, False)) for k, w in enumerate(wins))


# ---------------------------------------------------------------------------------------------------------------- python

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
def test_gpu_decoder_crop_batch_rate(f32):
    """windows in frames over all the files, whatever their channel count and rate"""
    import torch
    from libacm_amd import batch
    fs = DR.files()
    files = [f.data for f in fs]
    dec = batch.GpuDecoder(0, parse=capi.PARSE_DEVICE, dtype=torch.float32 if f32 else torch.int16)
    try:
        index = batch.build_index(files, threads=2)
        T = 50
        assert [batch.source_frames(T, r, DR.RATE) for r in (11025, 22050, 44100, 16000)] == [25, 50, 100, 36]
        windows = [(0, 0, 25), (1, 37, 25), (2, 300, 41), (3, fs[3].words // 2 - 10, T), (4, 3, 100), (5, 511, 1), (6, 9, 36), (7, 0, 5), (8, 0, T),
                   (9, 0, 5), (10, 0, 5), (11, fs[11].words - 20, 100), (5, 900, 99), (6, 77, 0), (0, fs[0].words - 3, 25)]
        for channels in (1, 2):
            for planar in (True, False):
                batch_t, frames, st = dec.crop_batch(files, windows, T, channels=channels, planar=planar, index=index, mix=True, rate=DR.RATE)
                n = len(windows)
                assert batch_t.dtype == dec.dtype and batch_t.is_cuda and tuple(batch_t.shape) == ((n, channels, T) if planar else (n, T, channels))
                got = batch_t.cpu().numpy().reshape(n, -1)
                for k, (f, a, m) in enumerate(windows):
                    c = DR.chans_of(f, channels)
                    want = DR.row_of(f, a * c, m * c, channels, T, planar, True)
                    assert frames[k] == DR.frames_out(f, a * c, m * c, channels, True), (k, frames[k])
                    if f == 8:
                        assert st[k] == capi.ERR_ARG and frames[k] == 0
                    assert np.array_equal(got[k].view(np.uint8), (DC.as_f32(want) if f32 else want).view(np.uint8)), (k, channels, planar)
                assert frames[:5] == [50, 50, 41, 10, 50] and frames[6] == 50 and frames[12] == 50 and frames[14] == 6
    finally:
        dec.dev.close()
