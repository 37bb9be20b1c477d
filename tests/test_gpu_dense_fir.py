"""acm_batch_decode_windows_overlay_fir on the GPU (include/acm_hip.h; libacm_amd/csrc/acm_batch_windows.cpp, acm_dense_fir.hip): source
rows convolved with an impulse response before the overlay call makes its rows from them.

Every call writes into the middle of a poisoned buffer with a guard row on either side (test_gpu_dense_overlay.poisoned): the guards
must keep the poison, and the rows, the gains and the energies must be the model's exactly - the operation is defined on integers, so
there is no tolerance.  The handle's fill mode is on (helpers): a filtered row the kernel did not write in full, or an input it read
from a place the gather launch did not write, shows up as 0xA5A5.

Expected rows: tests/dense_fir.py (tests/test_dense_fir.py holds the case list to what it has to reach).  Every test here calls
acm_batch_decode_windows_overlay_fir, which the library did not have before."""
import numpy as np
import pytest

import dense_fir as DF
import dense_overlay as DO
import helpers  # noqa: F401  (the fill mode of the handle, as in every module of GPU tests)
from libacm_amd import capi
from test_gpu_dense_crops import BOTH, POISON
from test_gpu_dense_overlay import check_rows, poisoned

pytestmark = pytest.mark.gpu

COUNTS = ("samples", "device_parsed", "host_parsed", "h2d_bytes", "blocks_parsed")


def call_kw(case, f32, parse):
    return dict(channels=case.channels, planar=case.planar, f32=f32, parse=parse, threads=4, mix=True, rate=DO.RATE, speeds=case.speeds)


def run(dev, case, f32, parse, shift=0, records=None, check=True, fir=None, **kw):
    """one call of the case -> (rows as written, statuses, words, offsets, gains, timing[, rc]); fir: other responses / of_window /
    ... than the case's own"""
    records = case.records if records is None else records
    fir = dict(responses=case.responses, of_window=case.of_window) if fir is None else fir
    got, res = poisoned(dev, len(records), case.row, f32, shift, lambda d, words: capi.batch_decode_windows_overlay_fir(
        dev, DF.data(), DF.index(), case.windows, records, d, words, case.frames, check=check, **fir, **call_kw(case, f32, parse), **kw))
    return (got,) + tuple(res)


def run_overlay(dev, case, f32, parse):
    """the same arguments through acm_batch_decode_windows_overlay"""
    got, res = poisoned(dev, len(case.records), case.row, f32, 0, lambda d, words: capi.batch_decode_windows_overlay(
        dev, DF.data(), DF.index(), case.windows, case.records, d, words, case.frames, **call_kw(case, f32, parse)))
    return (got,) + tuple(res)


def pick(frames, channels, planar=False):
    return next(c for c in DF.cases() if (c.frames, c.channels, c.planar) == (frames, channels, planar))


# ---------------------------------------------------------------------------------------------------------------- expected rows

@pytest.mark.parametrize("parse", BOTH, ids=["host", "device"])
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("case", DF.cases(), ids=lambda c: c.name)
def test_expected_rows(dev, case, f32, parse):
    got, st, words, offsets, gains, tm = run(dev, case, f32, parse)
    check_rows(case, got, gains, f32)
    for k in range(len(case.windows)):
        assert (words[k], st[k]) == case.expect(k), (k, case.windows[k], words[k], st[k])
    assert offsets == [(0, 0, 0)] * len(case.windows)
    # the rows of the identity responses are the dry row's, byte for byte
    at = {rec[0]: r for r, rec in enumerate(case.records) if rec[1] is None and rec[2] == 4096}
    assert got[at[DF.SAME0]].tobytes() == got[at[DF.SAME1]].tobytes() == got[at[DF.DRY]].tobytes()


def test_records_come_back_with_the_callers_rows(dev):
    """the table that is uploaded names the filtered rows; the caller's records keep their own a and b"""
    case = pick(64, 2)
    got, (st, words, offsets, table, tm) = poisoned(dev, len(case.records), case.row, False, 0, lambda d, n: capi.batch_decode_windows_overlay_fir(
        dev, DF.data(), DF.index(), case.windows, case.records, d, n, case.frames, responses=case.responses, of_window=case.of_window,
        result_table=True, **call_kw(case, False, capi.PARSE_HOST)))
    assert table["a"].tolist() == [rec[0] for rec in case.records]
    assert table["b"].tolist() == [capi.OVERLAY_NONE if rec[1] is None else rec[1] for rec in case.records]
    want = case.rows()[1]
    assert list(zip(table["gain"].tolist(), table["energy_a"].tolist(), table["energy_b"].tolist())) == want


# ---------------------------------------------------------------------------------------------------------------- an odd element offset

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("case", [c for c in DF.cases() if c.frames in (37, 6151) and not c.planar], ids=lambda c: c.name)
def test_tensor_one_element_behind_a_line(dev, case, f32):
    per_line = 4 if f32 else 8
    shift = (1 - case.row) % per_line
    assert (case.row + shift) % per_line == 1
    got, st, words, offsets, gains, tm = run(dev, case, f32, capi.PARSE_DEVICE, shift=shift)
    check_rows(case, got, gains, f32)


# ---------------------------------------------------------------------------------------------------------------- nothing to filter

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("case", [pick(2100, 1), pick(37, 2, True)], ids=lambda c: c.name)
def test_without_responses_the_call_is_the_overlay_call(dev, case, f32):
    """no acm_fir_opts, no responses, every window ACM_FIR_NONE: the output, the gains and the timing's counts of
    acm_batch_decode_windows_overlay for the same arguments, byte for byte"""
    want = run_overlay(dev, case, f32, capi.PARSE_DEVICE)
    for fir in (dict(no_fir=True), dict(responses=[], of_window=None), dict(responses=case.responses, of_window=[None] * len(case.windows))):
        got = run(dev, case, f32, capi.PARSE_DEVICE, fir=fir)
        assert got[0].tobytes() == want[0].tobytes() and got[1:5] == want[1:5], sorted(fir)
        assert [getattr(got[5], n) for n in COUNTS] == [getattr(want[5], n) for n in COUNTS], sorted(fir)


@pytest.mark.parametrize("case", [pick(6151, 1), pick(2100, 2), pick(37, 2, True)], ids=lambda c: c.name)
def test_the_identity_response_changes_nothing(dev, case):
    want = run_overlay(dev, case, False, capi.PARSE_HOST)
    for p in (DF.R_ONE, DF.R_UNITY14):
        got = run(dev, case, False, capi.PARSE_HOST, fir=dict(responses=case.responses, of_window=[p] * len(case.windows)))
        assert got[0].tobytes() == want[0].tobytes() and got[1:5] == want[1:5], p


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_refused_calls_write_nothing(dev):
    case = pick(64, 1)
    nwin = len(case.windows)
    good, of = case.responses, case.of_window
    h = good[DF.R_THREE][0]
    over = np.full(257, 255, np.int16)
    over[0] = 256

    def swap(p, r):
        return [r if q == p else x for q, x in enumerate(good)]
    for what, kw in (("a record beyond the windows", dict(records=case.records[:4] + [(nwin, None, 0, 0, 0)])),
                     ("an unknown dense flag", dict(dense_flags=64)),
                     ("no responses", dict(fir=dict(responses=None, of_window=of, nresp=3))),
                     ("no of_window", dict(fir=dict(responses=good, of_window=None))),
                     ("an entry == nresp", dict(fir=dict(responses=good, of_window=[len(good)] + of[1:]))),
                     ("reserved in the options", dict(fir=dict(responses=good, of_window=of, fir_reserved=1))),
                     ("no taps", dict(fir=dict(responses=swap(DF.R_THREE, (None, 0, 0)), of_window=of))),
                     ("delay == ntaps", dict(fir=dict(responses=swap(DF.R_THREE, (h, 3, 15)), of_window=of))),
                     ("shift 31", dict(fir=dict(responses=swap(DF.R_THREE, (h, 1, 31)), of_window=of))),
                     ("reserved in a response", dict(fir=dict(responses=swap(DF.R_THREE, (h, 1, 15, 1)), of_window=of))),
                     ("32769 taps", dict(fir=dict(responses=swap(DF.R_THREE, (np.zeros(32769, np.int16), 1, 15)), of_window=of))),
                     ("sum |h| 65536", dict(fir=dict(responses=swap(DF.R_THREE, (over, 1, 15)), of_window=of)))):
        got, *_, rc = run(dev, case, False, capi.PARSE_HOST, check=False, **kw)
        assert rc == capi.ERR_ARG, (what, rc)
        assert (got == POISON * 0x101).all(), what
    # one tap more than 2^22 in the responses the windows name: 128 of 32768 taps and the identity, over the case's windows in turn
    wins, speeds = [case.windows[k % nwin] for k in range(129)], [case.speeds[k % nwin] for k in range(129)]
    got, res = poisoned(dev, 4, case.row, False, 0, lambda d, n: capi.batch_decode_windows_overlay_fir(
        dev, DF.data(), DF.index(), wins, case.records[:4], d, n, case.frames, responses=[(np.ones(32768, np.int16), 0, 0)] * 128 + [good[DF.R_ONE]],
        of_window=list(range(129)), check=False, **dict(call_kw(case, False, capi.PARSE_HOST), speeds=speeds)))
    assert res[-1] == capi.ERR_ARG and (got == POISON * 0x101).all()
    assert capi.batch_decode_windows_overlay_fir(None, DF.data(), DF.index(), case.windows, case.records, 0, 0, case.frames, responses=good,
                                                 of_window=of, check=False)[-1] == capi.ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------------------------- launch caps

@pytest.mark.parametrize("grid", [1, 2, 3])
@pytest.mark.parametrize("case", [c for c in DF.cases() if c.frames == 6151], ids=lambda c: c.name)
def test_a_capped_grid_strides_over_the_rest(dev, case, grid):
    """the handle's dense grid cap at 1, 2 and 3 workgroups: every dense kernel of the call strides over its work; the rows are the
    same, and the cap is what it was afterwards"""
    was = dev.set_launch_caps(None)
    dev.set_launch_caps(was)
    with dev.launch_caps(dense_grid=grid):
        got, st, words, offsets, gains, tm = run(dev, case, False, capi.PARSE_HOST)
    check_rows(case, got, gains, False)
    now = dev.set_launch_caps(None)
    dev.set_launch_caps(now)
    assert now.as_dict() == was.as_dict()


# ---------------------------------------------------------------------------------------------------------------- python

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
def test_gpu_decoder_crop_overlay_with_reverb(f32):
    """speech windows with a response each or none, noise windows, Overlay(k, b=N + k, snr_db=10): torch tensors end to end, `out`
    included; the quantised responses through the model"""
    import torch
    import dense_crops as DC
    import dense_resample as DR
    from libacm_amd import batch
    files = [f.data for f in DR.files()]
    dec = batch.GpuDecoder(0, parse=capi.PARSE_DEVICE, dtype=torch.float32 if f32 else torch.int16)
    try:
        index = batch.build_index(files, threads=2)
        T, N = 50, 3
        speech = [(2, 10, T), (3, 7, T), (6, 30, batch.source_frames(T, 16000, DR.RATE, (9, 10)))]
        noise = [(0, 5, batch.source_frames(T, 11025, DR.RATE)), (5, 9, batch.source_frames(T, 44100, DR.RATE)), (2, 500, 20)]
        speed = [None, None, (9, 10), None, None, None]
        rng = np.random.default_rng(0xF1B)
        rir = rng.standard_normal(300) * np.exp(-np.arange(300) / 40.0)
        responses = [batch.Response(rir), batch.Response([0.1, 1.0, -0.4, 0.2]), batch.Response.raw([1], 0, 0)]
        reverb = [0, 1, 0, None, 2, None]
        rows = [batch.Overlay(k, b=N + k, snr_db=10) for k in range(N)] + [batch.Overlay(1, vol_db=-6), batch.Overlay(0, b=5, gain_db=-12, vol_db=3)]
        for channels, planar in ((1, True), (2, True), (2, False)):
            out = dec.empty(len(rows) * channels * T + 5)
            for given in (None, out):
                batch_t, gains, frames, st = dec.crop_overlay(files, speech + noise, rows, T, channels=channels, planar=planar, index=index, out=given,
                                                              mix=True, rate=DR.RATE, speed=speed, responses=responses, reverb=reverb)
                assert batch_t.dtype == dec.dtype and batch_t.is_cuda
                assert tuple(batch_t.shape) == ((len(rows), channels, T) if planar else (len(rows), T, channels))
                assert given is None or batch_t.data_ptr() == out.data_ptr()
                src = []
                for (f, a, m), s, p in zip(speech + noise, speed, reverb):
                    c = DR.chans_of(f, channels)
                    row = DO.DS.row_of(f, a * c, m * c, s, channels, T, planar, True, DR.RATE)
                    src.append(row if p is None else DF.filtered(row, channels, T, planar, responses[p].record)[0])
                got = batch_t.cpu().numpy().reshape(len(rows), -1)
                for r, row in enumerate(rows):
                    want, g = DO.row_of(src, row.record())
                    assert np.array_equal(got[r].view(np.uint8), (DC.as_f32(want) if f32 else want).view(np.uint8)), (r, channels, planar)
                    assert gains[r] == g, (r, gains[r], g)
                assert st == [0] * 6 and frames[:2] == [T, T] and frames[5] == 20
        # responses without reverb: nothing is filtered; reverb without responses, or of another length, is the caller's mistake
        dry = dec.crop_overlay(files, speech + noise, rows, T, index=index, mix=True, rate=DR.RATE, speed=speed)
        same = dec.crop_overlay(files, speech + noise, rows, T, index=index, mix=True, rate=DR.RATE, speed=speed, responses=responses)
        assert torch.equal(dry[0], same[0]) and dry[1:] == same[1:]
        with pytest.raises(ValueError):
            dec.crop_overlay(files, speech + noise, rows, T, index=index, mix=True, rate=DR.RATE, speed=speed, reverb=reverb)
        with pytest.raises(ValueError):
            dec.crop_overlay(files, speech + noise, rows, T, index=index, mix=True, rate=DR.RATE, speed=speed, responses=responses, reverb=reverb[:3])
    finally:
        dec.dev.close()
