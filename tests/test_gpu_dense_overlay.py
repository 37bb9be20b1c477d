"""acm_batch_decode_windows_overlay on the GPU (include/acm_hip.h; libacm_amd/csrc/acm_batch_windows.cpp, acm_dense_overlay.hip):
volume, and a second crop laid over the first at a signal-to-noise ratio, as rows of one tensor.

Every call writes into the middle of a poisoned buffer with a guard row on either side: the guards must keep the poison, and the rows,
the gains and the energies must be the model's exactly - the operation is defined on integers, so there is no tolerance.  The handle's
fill mode is on (helpers): a kernel that reads a place of the source arena the gather launch did not write shows up as 0xA5A5.

Expected rows: tests/dense_overlay.py (source rows from tests/dense_speed.py's model of the dense call, combined by the contract's
lines; tests/test_dense_overlay.py holds the gain to the integer model and the case list to what it has to reach).  Every test here
calls acm_batch_decode_windows_overlay, which the library did not have before."""
import numpy as np
import pytest

import dense_crops as DC
import dense_overlay as DO
import dense_resample as DR
import helpers  # noqa: F401  (the fill mode of the handle, as in every module of GPU tests)
from libacm_amd import capi
from test_gpu_dense_crops import BOTH, POISON, same

pytestmark = pytest.mark.gpu

_dense = {}


def data_and_index():
    return [f.data for f in DR.files()], DC.index_of(DR.files())


def poisoned(dev, n, R, f32, shift, call):
    """call(pointer to n rows, elements) with the rows in a poisoned buffer: a guard row, `shift` elements, the n rows, a guard row ->
    (the n rows as written, what call returned); everything around the rows must come back as poison"""
    unit, dt = (4, np.uint32) if f32 else (2, np.uint16)
    total = (n + 2) * R + shift
    d = dev.malloc(total * unit)
    try:
        assert d % 256 == 0
        dev.memset(d, POISON, total * unit)
        res = call(d + (R + shift) * unit, n * R)
        raw = np.zeros(total, dtype=dt)
        dev.download(raw, d)
    finally:
        dev.free(d)
    poison = np.frombuffer(bytes([POISON]) * unit, dtype=dt)[0]
    assert (raw[:R + shift] == poison).all(), "the call wrote in front of its tensor"
    assert (raw[total - R:] == poison).all(), "the call wrote behind its tensor"
    return raw[R + shift:total - R].reshape(n, R), res


def run(dev, case, f32, parse, shift=0, records=None, check=True, **kw):
    """one overlay call of the case -> (rows as written, statuses, words, offsets, gains, timing[, rc])"""
    files, index = data_and_index()
    records = case.records if records is None else records
    n = len(records)
    got, res = poisoned(dev, n, case.row, f32, shift, lambda d, words: capi.batch_decode_windows_overlay(
        dev, files, index, case.windows, records, d, words, case.frames, channels=case.channels, planar=case.planar, f32=f32, parse=parse,
        threads=4, mix=True, rate=DO.RATE, speeds=case.speeds, check=check, **kw))
    return (got,) + tuple(res)


def dense_call(dev, case, f32, parse):
    """(rows, statuses, words) of acm_batch_decode_windows_dense for the case's windows: once per case, type and parser"""
    key = (case.name, f32, parse)
    if key not in _dense:
        files, index = data_and_index()
        got, (st, words, tm) = poisoned(dev, len(case.windows), case.row, f32, 0, lambda d, n: capi.batch_decode_windows_dense(
            dev, files, index, case.windows, d, n, case.frames, channels=case.channels, planar=case.planar, f32=f32, parse=parse, threads=4,
            mix=True, rate=DO.RATE, speeds=case.speeds))
        _dense[key] = (got, st, words, tm)
    return _dense[key]


def check_rows(case, got, gains, f32):
    want, want_gains = case.rows()
    for r in range(len(case.records)):
        if not same(got[r], want[r], f32):
            ref = DC.as_f32(want[r]).view(np.uint32) if f32 else want[r].view(np.uint16)
            bad = np.nonzero(got[r] != ref)[0]
            raise AssertionError("row %d, record %r: %d of %d elements differ, the first at %d" % (r, case.records[r], bad.size, got[r].size, int(bad[0])))
        assert gains[r] == want_gains[r], (r, case.records[r], gains[r], want_gains[r])


# ---------------------------------------------------------------------------------------------------------------- expected rows

@pytest.mark.parametrize("parse", BOTH, ids=["host", "device"])
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("case", DO.cases(), ids=lambda c: c.name)
def test_expected_rows(dev, case, f32, parse):
    got, st, words, offsets, gains, tm = run(dev, case, f32, parse)
    check_rows(case, got, gains, f32)
    for k in range(len(case.windows)):
        assert (words[k], st[k]) == case.expect(k), (k, case.windows[k], words[k], st[k])
    assert offsets == [(0, 0, 0)] * len(case.windows)
    # statuses, words and the blocks parsed are the dense call's for the same windows; the identity rows are its rows, byte for byte
    rows, d_st, d_words, d_tm = dense_call(dev, case, f32, parse)
    assert st == d_st and words == d_words and (tm.blocks_parsed, tm.samples) == (d_tm.blocks_parsed, d_tm.samples)
    assert case.frames < 37 or (tm.device_parsed > 0) == (parse == capi.PARSE_DEVICE)
    ident = [(r, rec[0]) for r, rec in enumerate(case.records) if rec[1] is None and rec[2] == 4096]
    assert len(ident) >= len(case.windows) - 1
    for r, a in ident:
        assert got[r].tobytes() == rows[a].tobytes(), (r, a)


# ---------------------------------------------------------------------------------------------------------------- an odd element offset

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("case", [c for c in DO.cases() if c.frames in (37, 6151) and not c.planar], ids=lambda c: c.name)
def test_tensor_one_element_behind_a_line(dev, case, f32):
    """the tensor begins one element behind a 16-byte line: every row has single outputs in front of its first line"""
    per_line = 4 if f32 else 8
    shift = (1 - case.row) % per_line
    assert (case.row + shift) % per_line == 1
    got, st, words, offsets, gains, tm = run(dev, case, f32, capi.PARSE_DEVICE, shift=shift)
    check_rows(case, got, gains, f32)


# ---------------------------------------------------------------------------------------------------------------- refusals and no rows

def test_refused_calls_write_nothing(dev):
    case = next(c for c in DO.cases() if c.frames == 64 and c.channels == 1)
    good = case.records[:6]
    nwin = len(case.windows)
    for what, records, kw in (("a == nwin", good + [(nwin, None, 0, 0, 0)], {}),
                              ("b == nwin", good + [(0, nwin, 0, 65536, 0)], {}),
                              ("reserved", good + [(0, 1, 0, 65536, 0, 1)], {}),
                              ("an absolute gain above G_MAX", good + [(0, 1, 0, 0, 32769)], {}),
                              ("an unknown dense flag", good, dict(dense_flags=64)),
                              ("speeds without ACM_DENSE_RESAMPLE", good, dict(dense_flags=capi.DENSE_SPEED))):
        got, st, words, offsets, gains, tm, rc = run(dev, case, False, capi.PARSE_HOST, records=records, check=False, **kw)
        assert rc == capi.ERR_ARG, (what, rc)
        assert (got == POISON * 0x101).all(), what
    files, index = data_and_index()
    # a tensor one element short, no table for rows, no device
    got, res = poisoned(dev, len(good), case.row, False, 0, lambda d, n: capi.batch_decode_windows_overlay(
        dev, files, index, case.windows, good, d, n - 1, case.frames, mix=True, rate=DO.RATE, speeds=case.speeds, check=False))
    assert res[-1] == capi.ERR_ARG and (got == POISON * 0x101).all()
    got, res = poisoned(dev, 2, case.row, False, 0, lambda d, n: capi.batch_decode_windows_overlay(
        dev, files, index, case.windows, None, d, n, case.frames, mix=True, rate=DO.RATE, speeds=case.speeds, check=False, nrows=2))
    assert res[-1] == capi.ERR_ARG and (got == POISON * 0x101).all()
    assert capi.batch_decode_windows_overlay(None, files, index, case.windows, good, 0, 0, case.frames, check=False)[-1] == capi.ERR_NO_DEVICE


def test_no_rows_writes_nothing(dev):
    case = next(c for c in DO.cases() if c.frames == 37 and c.channels == 2 and c.planar)
    got, st, words, offsets, gains, tm = run(dev, case, False, capi.PARSE_DEVICE, records=[])
    assert got.size == 0 and gains == []
    assert [(words[k], st[k]) for k in range(len(case.windows))] == [case.expect(k) for k in range(len(case.windows))]


# ---------------------------------------------------------------------------------------------------------------- python

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
def test_gpu_decoder_crop_overlay(f32):
    """speech windows, noise windows, and Overlay(k, b=N + k, snr_db=10): torch tensors end to end, `out` included"""
    import torch
    from libacm_amd import batch
    files = [f.data for f in DR.files()]
    dec = batch.GpuDecoder(0, parse=capi.PARSE_DEVICE, dtype=torch.float32 if f32 else torch.int16)
    try:
        index = batch.build_index(files, threads=2)
        T, N = 50, 3
        speech = [(2, 10, T), (3, 7, T), (6, 30, batch.source_frames(T, 16000, DR.RATE, (9, 10)))]
        noise = [(0, 5, batch.source_frames(T, 11025, DR.RATE)), (5, 9, batch.source_frames(T, 44100, DR.RATE)), (2, 500, 20)]
        speed = [None, None, (9, 10), None, None, None]
        rows = [batch.Overlay(k, b=N + k, snr_db=10) for k in range(N)] + [batch.Overlay(1, vol_db=-6), batch.Overlay(0, b=5, gain_db=-12, vol_db=3)]
        for channels, planar in ((1, True), (2, True), (2, False)):
            out = dec.empty(len(rows) * channels * T + 5)
            for given in (None, out):
                res = dec.crop_overlay(files, speech + noise, rows, T, channels=channels, planar=planar, index=index, out=given, mix=True,
                                       rate=DR.RATE, speed=speed)
                batch_t, gains, frames, st = res
                assert batch_t.dtype == dec.dtype and batch_t.is_cuda
                assert tuple(batch_t.shape) == ((len(rows), channels, T) if planar else (len(rows), T, channels))
                assert given is None or batch_t.data_ptr() == out.data_ptr()
                src = []
                for (f, a, m), s in zip(speech + noise, speed):
                    c = DR.chans_of(f, channels)
                    src.append(DO.DS.row_of(f, a * c, m * c, s, channels, T, planar, True, DR.RATE))
                got = batch_t.cpu().numpy().reshape(len(rows), -1)
                for r, row in enumerate(rows):
                    want, g = DO.row_of(src, row.record())
                    assert np.array_equal(got[r].view(np.uint8), (DC.as_f32(want) if f32 else want).view(np.uint8)), (r, channels, planar)
                    assert gains[r] == g, (r, gains[r], g)
                assert st == [0] * 6 and frames[:2] == [T, T] and frames[5] == 20 and all(0 < n <= T for n in frames)
        with pytest.raises(ValueError):
            dec.crop_overlay(files, speech + noise, rows, T, index=index, speed=speed)
    finally:
        dec.dev.close()
