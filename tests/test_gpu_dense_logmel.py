"""acm_batch_decode_windows_logmel on the GPU (include/acm_hip.h; libacm_amd/csrc/acm_batch_windows.cpp, acm_dense_feat.hip): the
logarithm of the mel features of acm_batch_decode_windows_features, an integer one, floored, clamped to its row's maximum and scaled
in the same call.

Every call writes into the middle of a poisoned buffer with guards on either side (tests/test_gpu_dense_feat.py's harness): the guards
must keep the poison, and every element must be the model's bit for bit - the result is defined on integers and every output is an
exact float32, so there is no tolerance.  The handle's fill mode is on (helpers).

Expected values: tests/dense_logmel.py (tests/test_dense_logmel.py holds the case list to what it has to reach).  Every test here
calls acm_batch_decode_windows_logmel, which the library did not have before."""
import math

import numpy as np
import pytest

import dense_feat as M
import dense_logmel as G
import helpers  # noqa: F401  (the fill mode of the handle, as in every module of GPU tests)
from libacm_amd import capi
from test_gpu_dense_crops import BOTH
from test_gpu_dense_feat import POISON32, call_kw, check_features, guarded
from test_gpu_dense_feat import run as run_linear

pytestmark = pytest.mark.gpu


def run(dev, lc, parse, shift=0, log="case", bank=None, check=True, words=None, **kw):
    """one call of the case -> (the elements as written, uint32, statuses, words, offsets, gains, timing[, rc])"""
    case = lc.case
    n = len(case.records) * case.bank.n_mels * case.F
    got, res = guarded(dev, n, shift, lambda d, room: capi.batch_decode_windows_logmel(
        dev, M.data(), M.index(), case.windows, case.records, d, room if words is None else words, case.frames,
        case.bank.record if bank is None else bank, lc.scale.record if log == "case" else log, check=check, responses=case.responses,
        of_window=case.of_window, **dict(call_kw(case, parse), **kw)))
    return (got,) + tuple(res)


def check_logmel(lc, got, gains):
    want = lc.logmel()[0]
    want_gains = lc.case.rows()[1]
    got = got.reshape(want.shape)
    for r in range(len(lc.case.records)):
        if got[r].tobytes() != want[r].view(np.uint32).tobytes():
            bad = np.argwhere(got[r] != want[r].view(np.uint32))
            at = tuple(int(v) for v in bad[0])
            raise AssertionError("%s, row %d, record %r: %d of %d elements differ, the first at %r: %08x for %08x" % (
                lc.name, r, lc.case.records[r], len(bad), got[r].size, at, int(got[r][at]), int(want[r].view(np.uint32)[at])))
        assert gains[r] == want_gains[r], (r, lc.case.records[r], gains[r], want_gains[r])


# ---------------------------------------------------------------------------------------------------------------- expected values

@pytest.mark.parametrize("parse", BOTH, ids=["host", "device"])
@pytest.mark.parametrize("lc", G.cases(), ids=lambda c: c.name)
def test_expected_logmel(dev, lc, parse):
    got, st, words, offsets, gains, tm = run(dev, lc, parse)
    check_logmel(lc, got, gains)
    case = lc.case
    for k in range(len(case.windows)):
        assert (words[k], st[k]) == case.expect(k), (k, case.windows[k], words[k], st[k])
    assert offsets == [(0, 0, 0)] * len(case.windows)


# ---------------------------------------------------------------------------------------------------------------- an odd element offset

@pytest.mark.parametrize("lc", [G.pick("t2100_d512_h160_b80_whisper"), G.pick("t6151_d128_h37_b128_whole_db_top80"),
                                G.pick("t37_d512_h37_b80_tm_whisper")], ids=lambda c: c.name)
def test_tensor_one_element_behind_a_line(dev, lc):
    assert lc.scale.top
    got, st, words, offsets, gains, tm = run(dev, lc, capi.PARSE_DEVICE, shift=1)
    check_logmel(lc, got, gains)


# ---------------------------------------------------------------------------------------------------------------- launch caps

@pytest.mark.parametrize("grid", [1, 2, 3])
@pytest.mark.parametrize("lc", [G.pick("t2100_d128_hN_b23_whisper"), G.pick("tail_t6151_d128_h37_b128_whole_db_top30")], ids=lambda c: c.name)
def test_a_capped_grid_strides_over_the_rest(dev, lc, grid):
    """one, two and three workgroups over all tiles of all rows - the atomics of one workgroup into several rows' maxima - and over
    all elements of the second pass"""
    assert lc.scale.top and len(lc.case.records) * -(-lc.case.F // M.TILE) > 3 and lc.logmel()[0].size > 3 * 256
    with dev.launch_caps(dense_grid=grid):
        got, st, words, offsets, gains, tm = run(dev, lc, capi.PARSE_HOST)
    check_logmel(lc, got, gains)


# ---------------------------------------------------------------------------------------------------------------- the table of maxima

def test_a_quiet_call_behind_a_loud_one(dev):
    """one handle, one bank, the same number of rows: the maxima of the loud call lie more than `top` above the quiet one's, so a
    table that the quiet call did not reset would clamp its rows to the loud call's"""
    loud, quiet = G.pick("loud_t2100_d128_hN_b23_db_top30"), G.pick("quiet_t2100_d128_hN_b23_db_top30")
    for lc in (loud, quiet, loud, quiet):
        got, st, words, offsets, gains, tm = run(dev, lc, capi.PARSE_HOST)
        check_logmel(lc, got, gains)


def test_the_linear_call_between_two_logmel_calls(dev):
    lc = G.pick("t2100_d512_h160_b80_whisper")
    plain = G.pick("t2100_d512_h160_b80_ln")
    for turn in range(2):
        got, st, words, offsets, gains, tm = run(dev, lc, capi.PARSE_HOST)
        check_logmel(lc, got, gains)
        lin = run_linear(dev, lc.case, capi.PARSE_HOST)
        check_features(lc.case, lin[0], lin[4])
        got, st, words, offsets, gains, tm = run(dev, plain, capi.PARSE_HOST)
        check_logmel(plain, got, gains)
    # what goes up is a features call's: the scale travels with the launch
    assert tm.h2d_bytes == lin[5].h2d_bytes


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_refused_calls_write_nothing(dev):
    lc = G.pick("t64_raw128_plus_whisper")
    case = lc.case
    good = list(lc.scale.record)
    FLAGS, FLOOR, MUL, OFF, TOP = range(5)

    def swap(i, v, base=good, reserved=0):
        return tuple(v if j == i else x for j, x in enumerate(base)) + (reserved,)
    notop = [0] + good[1:4] + [0]
    one = [0, -2177059, 1 << 24, 0, 0]
    bank = list(case.bank.record)
    scales = [("an unknown flag", swap(FLAGS, 3)), ("reserved", swap(None, None, reserved=1)),
              ("a floor below -64", swap(FLOOR, -G.FLOOR_MAX - 1)), ("a floor above 64", swap(FLOOR, G.FLOOR_MAX + 1)),
              ("a scale of 0", swap(MUL, 0)), ("a scale above 2^28", swap(MUL, G.MUL_MAX + 1)),
              ("a top above 128", swap(TOP, G.TOP_MAX + 1)), ("a top without the flag", swap(TOP, 1, notop)),
              ("an output that could reach 2^24", swap(OFF, (1 << 24) - 62 * 65536 - 1, one))]
    assert not any(G.check(log[:5], log[5]) for what, log in scales)
    refused = [(what, dict(log=log)) for what, log in scales]
    refused += [("no scale", dict(log=None)),
                ("a bank the features call refuses", dict(bank=tuple(bank[:3] + [4] + bank[4:]))),
                ("no bank", dict(no_bank=True)),
                ("two channels", dict(channels=2)),
                ("a tensor one element short", dict(words=len(case.records) * case.bank.n_mels * case.F - 1))]
    for what, kw in refused:
        res = run(dev, lc, capi.PARSE_HOST, check=False, **kw)
        assert res[-1] == capi.ERR_ARG, (what, res[-1])
        assert (res[0] == POISON32).all(), what
    # the boundaries beside them are taken
    for log in (swap(OFF, (1 << 24) - 62 * 65536 - 2, one), swap(TOP, G.TOP_MAX), swap(FLOOR, G.FLOOR_MAX)):
        assert G.check(log[:5], log[5])
        edge = G.LogCase(case, G.Scale("edge", *log[:5]))
        got, st, words, offsets, gains, tm = run(dev, edge, capi.PARSE_HOST)
        check_logmel(edge, got, gains)


# ---------------------------------------------------------------------------------------------------------------- python

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
def test_gpu_decoder_crop_features_log(f32):
    """GpuDecoder.crop_features(log=): torch tensors end to end, `out` given and not, for both dtypes of the decoder, against the model
    over the linear call's own bits (they determine E's 24 leading bits and its exponent, and so L) - and, loosely, against torch's
    logarithm of the linear call.  That bound is derived: frac lies at most 1.02 units of 2^-16 below the true log2 (tests/
    test_dense_logmel.py), which the scale multiplies by c * post_mul and rounds once more, half a unit of 2^-16 - c * 1.02 * 2^-16 +
    2^-17 for a post_mul of 1 -, and torch's logarithm is taken in float64 here, whose error at |log y| <= 64 is below 1e-12."""
    import torch
    import dense_resample as DR
    from libacm_amd import batch
    files = [f.data for f in DR.files()]
    dec = batch.GpuDecoder(0, parse=capi.PARSE_DEVICE, dtype=torch.float32 if f32 else torch.int16)
    try:
        index = batch.build_index(files, threads=2)
        T = 300
        wins = [(2, 10, T), (3, 7, T), (2, 500, 20)]
        rows = [batch.Overlay(0), batch.Overlay(1, b=0, snr_db=10), batch.Overlay(2, vol_db=-60), batch.Overlay(2)]
        bank = batch.MelBank(DR.RATE, 256, None, 100, 40)
        F = bank.frames(T)
        kw = dict(rows=rows, index=index, mix=True, rate=DR.RATE)
        lin, gains0, frames0, st0 = dec.crop_features(files, wins, T, bank, **kw)
        lin = lin.clone()
        bits = lin.cpu().numpy().view(np.uint32).astype(np.int64)
        # E's leading bit and mantissa from the float: y = m * 2^(e - 23), p - (75 - 2 n) = e
        e, m = (bits >> 23) - 127, (bits & 0x7FFFFF) | 0x800000
        assert (bits == 0).any() and (bits != 0).any()                     # a window of 20 samples: the frames behind them are silent
        out = torch.empty(len(rows) * bank.n_mels * F + 5, dtype=torch.float32, device="cuda:0")
        for scale, c, post in ((batch.LogScale(), math.log(2.0), 1.0), (batch.LogScale.whisper(), math.log10(2.0), 0.25),
                               (batch.LogScale("db", top=30.0, post_add=3.0), 10 * math.log10(2.0), 1.0)):
            s = G.Scale("s", *scale.record)
            L = np.where(bits != 0, np.maximum(e * 65536 + G.frac(m.astype(np.uint64))[0].astype(np.int64), s.floor_q16), s.floor_q16)
            if s.top:
                L = np.maximum(L, L.reshape(len(rows), -1).max(axis=1)[:, None, None] - s.top_q16)
            want = (G.scaled(L, s).astype(np.float64) / 65536.0).astype(np.float32)
            for given in (None, out):
                feats, gains, frames, st = dec.crop_features(files, wins, T, bank, out=given, log=scale, **kw)
                assert feats.dtype == torch.float32 and feats.is_cuda and tuple(feats.shape) == (len(rows), bank.n_mels, F)
                assert given is None or feats.data_ptr() == out.data_ptr()
                assert (gains, frames, st) == (gains0, frames0, st0)
                assert feats.cpu().numpy().tobytes() == want.tobytes(), scale.record
            # torch's way over the linear call
            floor = 2.0 ** (s.floor_q16 / 65536.0)
            x = torch.log2(torch.clamp(lin.double(), min=floor))
            if s.top:
                x = torch.maximum(x, x.amax(dim=(1, 2), keepdim=True) - s.top_q16 / 65536.0)
            x = x * (s.mul_q24 / 2.0 ** 24) + s.offset_q16 / 65536.0
            assert abs(s.mul_q24 / 2.0 ** 24 - c * post) < 2.0 ** -24
            bound = c * post * 1.02 * 2.0 ** -16 + 2.0 ** -17 + 1e-12 * 64
            err = float((feats.double() - x).abs().max())
            print("%r: largest distance to torch %.3g, bound %.3g" % (scale.record, err, bound))
            assert err <= bound, (scale.record, err, bound)
        with pytest.raises(ValueError):
            dec.crop_features(files, wins, T, bank, log=batch.LogScale("db", post_mul=2.0), **kw)
        with pytest.raises(ValueError):
            dec.crop_features(files, wins, T, bank, log=batch.LogScale.raw(0, top_q16=G.TOP_MAX + 1), **kw)
    finally:
        dec.dev.close()
