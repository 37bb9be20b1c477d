"""acm_batch_decode_windows_features on the GPU (include/acm_hip.h; libacm_amd/csrc/acm_batch_windows.cpp, acm_dense_feat.hip): mel
filterbank features of the rows acm_batch_decode_windows_overlay_fir would write, made on the matrix cores in the same call.

Every call writes float32 features into the middle of a poisoned buffer with guards on either side: the guards must keep the poison,
and the features, the gains and the energies must be the model's exactly - the result is defined on integers and every feature is an
exact float32, so there is no tolerance.  The handle's fill mode is on (helpers): a row the combine launch did not write in full into
the feature arena, or a sample the feature kernel read from a place nobody wrote, shows up as 0xA5A5.

Expected features: tests/dense_feat.py (tests/test_dense_feat.py holds the case list to what it has to reach).  Every test here calls
acm_batch_decode_windows_features, which the library did not have before."""
import numpy as np
import pytest

import dense_feat as M
import dense_fir as DF
import dense_overlay as DO
import helpers  # noqa: F401  (the fill mode of the handle, as in every module of GPU tests)
from libacm_amd import capi
from test_gpu_dense_crops import BOTH, POISON
from test_gpu_dense_overlay import poisoned

pytestmark = pytest.mark.gpu

GUARD = 256                             # float32 elements of poison on either side of the tensor
POISON32 = POISON * 0x01010101
COUNTS = ("samples", "device_parsed", "host_parsed", "blocks_parsed")


def call_kw(case, parse):
    return dict(channels=1, planar=False, parse=parse, threads=4, mix=True, rate=DO.RATE, speeds=case.speeds)


def guarded(dev, words, shift, call):
    """call(pointer, words) with `words` float32 elements, `shift` elements behind a 256-byte line, between two guards of poison ->
    (the elements as written, uint32; what call returned)"""
    total = 2 * GUARD + shift + words
    d = dev.malloc(total * 4)
    try:
        assert d % 256 == 0
        dev.memset(d, POISON, total * 4)
        res = call(d + (GUARD + shift) * 4, words)
        raw = np.zeros(total, dtype=np.uint32)
        dev.download(raw, d)
    finally:
        dev.free(d)
    assert (raw[:GUARD + shift] == POISON32).all(), "the call wrote in front of its tensor"
    assert (raw[GUARD + shift + words:] == POISON32).all(), "the call wrote behind its tensor"
    return raw[GUARD + shift:GUARD + shift + words], res


def run(dev, case, parse, shift=0, bank=None, check=True, records=None, fir=None, words=None, **kw):
    """one call of the case -> (features as written, uint32, statuses, words, offsets, gains, timing[, rc])"""
    bank = case.bank.record if bank is None else bank
    records = case.records if records is None else records
    fir = dict(responses=case.responses, of_window=case.of_window) if fir is None else fir
    n = len(records) * case.bank.n_mels * case.F
    got, res = guarded(dev, n, shift, lambda d, room: capi.batch_decode_windows_features(
        dev, M.data(), M.index(), case.windows, records, d, room if words is None else words, case.frames, bank, check=check, **fir,
        **call_kw(case, parse), **kw))
    return (got,) + tuple(res)


def check_features(case, got, gains):
    want, detail = case.features()
    want_gains = case.rows()[1]
    got = got.reshape(want.shape)
    for r in range(len(case.records)):
        if got[r].tobytes() != want[r].view(np.uint32).tobytes():
            bad = np.argwhere(got[r] != want[r].view(np.uint32))
            at = tuple(int(v) for v in bad[0])
            raise AssertionError("row %d, record %r: %d of %d features differ, the first at %r: %08x for %08x" % (
                r, case.records[r], len(bad), got[r].size, at, int(got[r][at]), int(want[r].view(np.uint32)[at])))
        assert gains[r] == want_gains[r], (r, case.records[r], gains[r], want_gains[r])


def pick(name):
    return next(c for c in M.cases() if c.name == name)


# ---------------------------------------------------------------------------------------------------------------- expected features

@pytest.mark.parametrize("parse", BOTH, ids=["host", "device"])
@pytest.mark.parametrize("case", M.cases(), ids=lambda c: c.name)
def test_expected_features(dev, case, parse):
    got, st, words, offsets, gains, tm = run(dev, case, parse)
    check_features(case, got, gains)
    for k in range(len(case.windows)):
        assert (words[k], st[k]) == case.expect(k), (k, case.windows[k], words[k], st[k])
    assert offsets == [(0, 0, 0)] * len(case.windows)
    # an all-zero row's features are +0.0, bit for bit
    zero = [r for r, rec in enumerate(case.records) if rec == M.ident(DF.BEHIND)]
    assert not zero or not got.reshape(len(case.records), -1)[zero[0]].any()


# ---------------------------------------------------------------------------------------------------------------- an odd element offset

@pytest.mark.parametrize("case", [pick("t2100_d512_h160_b80"), pick("t2100_d512_w400_h160_b80_tm"), pick("t6151_d128_h37_b128_whole")], ids=lambda c: c.name)
def test_tensor_one_element_behind_a_line(dev, case):
    got, st, words, offsets, gains, tm = run(dev, case, capi.PARSE_DEVICE, shift=1)
    check_features(case, got, gains)


# ---------------------------------------------------------------------------------------------------------------- the rows in the arena

@pytest.mark.parametrize("case", [pick("t37_d512_h37_b80_tm"), pick("t2100_d512_h160_b80"), pick("t6151_d512_h160_b80")], ids=lambda c: c.name)
def test_rows_are_the_overlay_fir_calls(dev, case):
    """the int16 rows in the feature arena, read through acmhip_device_arena_info, against what acm_batch_decode_windows_overlay_fir
    writes for the same arguments; and everything the two calls report"""
    n, R = len(case.records), case.frames
    want, res = poisoned(dev, n, R, False, 0, lambda d, words: capi.batch_decode_windows_overlay_fir(
        dev, M.data(), M.index(), case.windows, case.records, d, words, case.frames, responses=case.responses, of_window=case.of_window,
        **call_kw(case, capi.PARSE_HOST)))
    got = run(dev, case, capi.PARSE_HOST)
    slot, ptr, nbytes, is_host, fill = dev.arena_info()["D_FEAT"]
    assert ptr and not is_host and fill == 0xA5 and nbytes >= n * R * 2
    rows = np.zeros(n * R, dtype=np.uint16)
    dev.download(rows, ptr)
    assert rows.tobytes() == want.tobytes()
    assert want.view(np.int16).reshape(n, R).tobytes() == case.rows()[0].tobytes()
    assert got[1:5] == tuple(res[:4])
    assert [getattr(got[5], c) for c in COUNTS] == [getattr(res[4], c) for c in COUNTS]


# ---------------------------------------------------------------------------------------------------------------- launch caps

@pytest.mark.parametrize("grid", [1, 2, 3])
@pytest.mark.parametrize("case", [pick("t6151_d512_h160_b80"), pick("t2100_d128_hN_b23")], ids=lambda c: c.name)
def test_a_capped_grid_strides_over_the_rest(dev, case, grid):
    was = dev.set_launch_caps(None)
    dev.set_launch_caps(was)
    with dev.launch_caps(dense_grid=grid):
        got, st, words, offsets, gains, tm = run(dev, case, capi.PARSE_HOST)
    check_features(case, got, gains)
    now = dev.set_launch_caps(None)
    dev.set_launch_caps(now)
    assert now.as_dict() == was.as_dict()


# ---------------------------------------------------------------------------------------------------------------- the operand of the DFT

def test_each_call_gets_its_own_banks_operand(dev):
    """two banks of one n_fft on one handle, in turn and again: the DFT's operand is the one of the call's own cs"""
    plus, minus, mel = pick("t2100_raw128_plus"), pick("t2100_raw128_minus_tm"), pick("t2100_d128_hN_b23")
    first = {}
    for turn in range(2):
        for case in (plus, mel, minus, mel):
            got, st, words, offsets, gains, tm = run(dev, case, capi.PARSE_HOST)
            check_features(case, got, gains)
            assert first.setdefault(case.name, got.tobytes()) == got.tobytes()
    again = run(dev, mel, capi.PARSE_HOST)[0]
    assert again.tobytes() == first[mel.name]


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_refused_calls_write_nothing(dev):
    case = pick("t64_raw128_plus")
    b = case.bank
    good = list(b.record)
    N, H, B, FLAGS, WIN, CS, FIRST, COUNT, OFF, W = range(10)

    def swap(i, v):
        return tuple(v if j == i else x for j, x in enumerate(good))

    def table(i, at, v):
        a = np.array(good[i]).astype(np.int64)
        a[at] = v
        return swap(i, a)
    refused = [("a record beyond the windows", dict(records=case.records[:2] + [(len(case.windows), None, 0, 0, 0)])),
               ("two channels", dict(channels=2)),
               ("no bank", dict(no_bank=True)),
               ("a response the filter refuses", dict(fir=dict(responses=[(np.array([1], np.int16), 1, 0)], of_window=[None] * len(case.windows)))),
               ("n_fft 64", dict(bank=swap(N, 64))), ("n_fft 192", dict(bank=swap(N, 192))), ("n_fft 4096", dict(bank=swap(N, 4096))),
               ("hop 0", dict(bank=swap(H, 0))), ("hop N + 1", dict(bank=swap(H, 129))),
               ("no bands", dict(bank=swap(B, 0))),
               ("an unknown flag", dict(bank=swap(FLAGS, 4))),
               ("reserved", dict(bank=dict(zip(("n_fft", "hop", "n_mels", "flags", "window", "cs", "mel_first", "mel_count", "mel_off", "mel_w"), good), reserved=1))),
               ("a window value 32640", dict(bank=table(WIN, 5, 32640))), ("a negative window value", dict(bank=table(WIN, 127, -1))),
               ("a cosine 16385", dict(bank=table(CS, 0, 16385))), ("a cosine -16385", dict(bank=table(CS, 127, -16385))),
               ("a band past N / 2", dict(bank=table(FIRST, 2, 65))), ("a band one bin too long", dict(bank=table(COUNT, 1, 66))),
               ("a weight 32769", dict(bank=table(W, 64, 32769))),
               ("a tensor one element short", dict(words=len(case.records) * b.n_mels * case.F - 1))]
    refused += [("no %s" % name, dict(bank=swap(i, None))) for i, name in ((WIN, "window"), (CS, "cs"), (FIRST, "mel_first"), (COUNT, "mel_count"),
                                                                          (OFF, "mel_off"), (W, "mel_w"))]
    for what, kw in refused:
        kw = dict(kw)
        channels = kw.pop("channels", 1)
        got, res = guarded(dev, len(case.records) * b.n_mels * case.F, 0, lambda d, room: capi.batch_decode_windows_features(
            dev, M.data(), M.index(), case.windows, kw.get("records", case.records), d, kw.get("words", room), case.frames, kw.get("bank", b.record),
            check=False, no_bank=kw.get("no_bank", False), **kw.get("fir", dict(responses=case.responses, of_window=case.of_window)),
            **dict(call_kw(case, capi.PARSE_HOST), channels=channels)))
        assert res[-1] == capi.ERR_ARG, (what, res[-1])
        assert (got == POISON32).all(), what
    assert capi.batch_decode_windows_features(None, M.data(), M.index(), case.windows, case.records, 0, 0, case.frames, b.record,
                                              responses=case.responses, of_window=case.of_window, check=False)[-1] == capi.ERR_NO_DEVICE
    # the boundaries beside them are taken
    got, st, words, offsets, gains, tm = run(dev, case, capi.PARSE_HOST, bank=table(W, 64, 32768))
    check_features(case, got, gains)


# ---------------------------------------------------------------------------------------------------------------- python

@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
def test_gpu_decoder_crop_features(f32):
    """speech windows at a speed, with a response or dry, a stereo file mixed down, noise at an SNR: torch tensors end to end, `out`
    given and not, float32 whatever the decoder's dtype; the rows through tests/dense_overlay.py and tests/dense_fir.py"""
    import torch
    import dense_resample as DR
    from libacm_amd import batch
    files = [f.data for f in DR.files()]
    dec = batch.GpuDecoder(0, parse=capi.PARSE_DEVICE, dtype=torch.float32 if f32 else torch.int16)
    try:
        index = batch.build_index(files, threads=2)
        T, N = 300, 3
        speech = [(2, 10, T), (3, 7, T), (6, 30, batch.source_frames(T, 16000, DR.RATE, (9, 10)))]
        noise = [(0, 5, batch.source_frames(T, 11025, DR.RATE)), (5, 9, batch.source_frames(T, 44100, DR.RATE)), (2, 500, 20)]
        speed = [None, None, (9, 10), None, None, None]
        rng = np.random.default_rng(0xFEA7)
        responses = [batch.Response(rng.standard_normal(120) * np.exp(-np.arange(120) / 30.0)), batch.Response.raw([1], 0, 0)]
        reverb = [0, None, 0, None, 1, None]
        rows = [batch.Overlay(k, b=N + k, snr_db=10) for k in range(N)] + [batch.Overlay(1, vol_db=-6), batch.Overlay(0, b=5, gain_db=-12, vol_db=3)]
        src = []
        for (f, a, m), s, p in zip(speech + noise, speed, reverb):
            c = DR.chans_of(f, 1)
            row = DO.DS.row_of(f, a * c, m * c, s, 1, T, True, True, DR.RATE)
            src.append(row if p is None else DF.filtered(row, 1, T, True, responses[p].record)[0])
        for bank, model in ((batch.MelBank(DR.RATE, 256, None, 100, 40), M.design("a", DR.RATE, 256, None, 100, 40)),
                            (batch.MelBank(DR.RATE, 128, 100, 64, 23, 50.0, 7000.0, center=False, time_major=True),
                             M.design("b", DR.RATE, 128, 100, 64, 23, 50.0, 7000.0, flags=M.TIME_MAJOR))):
            F = bank.frames(T)
            assert F == model.frames(T) and all(np.array_equal(a, b) for a, b in zip(bank.record[4:], model.record[4:]))
            out = torch.empty(len(rows) * bank.n_mels * F + 3, dtype=torch.float32, device="cuda:0")
            for given in (None, out):
                feats, gains, frames, st = dec.crop_features(files, speech + noise, T, bank, rows=rows, index=index, out=given, mix=True, rate=DR.RATE,
                                                             speed=speed, responses=responses, reverb=reverb)
                assert feats.dtype == torch.float32 and feats.is_cuda
                assert tuple(feats.shape) == ((len(rows), F, bank.n_mels) if bank.time_major else (len(rows), bank.n_mels, F))
                assert given is None or feats.data_ptr() == out.data_ptr()
                got = feats.cpu().numpy()
                for r, row in enumerate(rows):
                    y, g = DO.row_of(src, row.record())
                    want = M.features(y, model)
                    want = want.T if bank.time_major else want
                    assert got[r].tobytes() == np.ascontiguousarray(want).tobytes(), (r, bank.n_fft)
                    assert gains[r] == g, (r, gains[r], g)
                assert st == [0] * 6 and frames[:2] == [T, T] and frames[5] == 20
        # rows=None: one Overlay(k) per window
        plain = dec.crop_features(files, speech + noise, T, bank, index=index, mix=True, rate=DR.RATE, speed=speed)
        named = dec.crop_features(files, speech + noise, T, bank, rows=[batch.Overlay(k) for k in range(6)], index=index, mix=True, rate=DR.RATE, speed=speed)
        assert tuple(plain[0].shape)[0] == 6 and torch.equal(plain[0], named[0]) and plain[1:] == named[1:]
        with pytest.raises(ValueError):
            dec.crop_features(files, speech + noise, T, bank, index=index, mix=True, rate=DR.RATE, speed=speed,
                              out=torch.empty(out.numel(), dtype=torch.int16, device="cuda:0"))
        with pytest.raises(ValueError):
            dec.crop_features(files, speech + noise, T, bank, index=index, mix=True, rate=DR.RATE, speed=speed, reverb=reverb)
    finally:
        dec.dev.close()
