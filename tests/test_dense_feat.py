"""Mel filterbank features from dense crop batches without a GPU: the device-free half of acm_batch_decode_windows_features
(libacm_amd/csrc/acm_feat_layout.cpp), the numpy model and the case list of tests/dense_feat.py.

  * acm_feat_design() against the model's own design, table by table; batch.MelBank on top of it.
  * acm_feat_bank_check(): every refusal with the boundary that passes beside it; batch.MelBank.raw.
  * acm_feat_frames() against the model.
  * the device-free half under AddressSanitizer and UBSan, as a program of its own (tests/native/feat_layout.cpp): the byte split,
    the partial sums' bounds, the join, the two-limb mel sum and trunc24 against 128 bits.
  * what the case list reaches, asserted on the model so that the GPU tests over the same list cannot pass vacuously.
  * the model is a mel spectrogram: against a float64 STFT and mel matrix in numpy.

The model against float64, measured here (seed 0xFEA7, a sine of amplitude 0.4 plus noise of 0.05, 16 000 samples at 16 kHz; the largest
relative error over the bands whose float64 energy is above 2^-40 of the row's largest; profiles/dense_feat_notes.txt):
    n_fft 512, hop 160, 80 bands, centred           1.04e-2
    n_fft 2048, hop 192, 128 bands, centred         1.78e-3
    n_fft 128, window 100, hop 64, 23 bands, whole  1.68e-2
The test asserts twice these: that covers another seed and cannot hide a wrong scale, which would be off by a factor of 2 at least."""
import os
import subprocess

import numpy as np
import pytest

import dense_feat as M
from libacm_amd import batch, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ("window", "cs", "mel_first", "mel_count", "mel_off", "mel_w")
DESIGNS = [(16000, 512, None, 160, 80, 0.0, None), (16000, 128, None, 128, 23, 0.0, None), (16000, 128, None, 1, 23, 100.0, 7000.0),
           (16000, 512, 400, 160, 80, 0.0, None), (16000, 2048, None, 192, 128, 0.0, None), (16000, 2048, None, 160, 1, 0.0, None),
           (16000, 128, None, 37, 128, 0.0, None), (22050, 256, None, 100, 40, 0.0, None), (22050, 128, 100, 64, 23, 50.0, 7000.0),
           (44100, 1024, 1000, 441, 64, 20.0, 20000.0), (8000, 256, 200, 80, 128, 0.0, 4000.0)]


# ---------------------------------------------------------------------------------------------------------------- the design

@pytest.mark.parametrize("args", DESIGNS, ids=lambda a: "r%d_n%d_w%s_h%d_b%d" % a[:5])
def test_design_is_the_models(args):
    want = M.design("m", *args)
    got = capi.feat_design(*args)
    for name, g, w in zip(TABLES, got, want.record[4:]):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        # one entry apart by one: a tie that two libms round apart - the message names it
        assert bad.size == 0, "%s[%d]: the library has %d, the model %d (%d entries differ)" % (name, bad[0], g[bad[0]], w[bad[0]], bad.size)
    assert capi.feat_bank_check(*want.record) == 0
    n_fft = args[1]
    assert got[0].max() == M.WINDOW_MAX and got[0].min() == 0 and got[1][0] == M.CS_ONE and got[1][n_fft // 2] == -M.CS_ONE
    assert int(got[4][-1]) + int(got[3][-1]) == got[5].size and got[5].max() <= M.W_ONE


def test_the_cases_designed_banks_are_the_librarys():
    seen = set()
    for case in M.cases():
        b = case.bank
        if b.name.startswith("d") and b.name not in seen:
            seen.add(b.name)
            assert capi.feat_bank_check(*b.record) == 0, b.name
    assert len(seen) >= 8


def test_design_refusals():
    for kw in (dict(n_fft=500), dict(n_fft=64), dict(n_fft=4096), dict(win_length=513), dict(win_length=0), dict(hop=0), dict(hop=513), dict(n_mels=0),
               dict(n_mels=129), dict(f_min=-1.0), dict(f_min=4000.0, f_max=4000.0), dict(f_max=8000.5), dict(flags=4)):
        with pytest.raises(ValueError):
            capi.feat_design(16000, **kw)
    capi.feat_design(16000, hop=512, n_mels=128, f_max=8000.0, flags=3)


def test_mel_bank():
    b = batch.MelBank(16000)
    m = M.design("m", 16000)
    assert (b.n_fft, b.hop, b.n_mels, b.center, b.time_major) == (512, 160, 80, True, False)
    assert all(np.array_equal(x, y) for x, y in zip(b.record[4:], m.record[4:]))
    assert b.frames(16000) == 101 and batch.MelBank(16000, center=False).frames(16000) == 97
    r = batch.MelBank.raw(128, 64, *M.raw_bound("r", 128, 64, 1, 1).record[4:], center=True, time_major=True)
    assert (r.n_mels, r.flags, r.frames(64)) == (4, 3, 2)
    good = list(M.raw_bound("r", 128, 64, 1, 1).record[4:])
    for i, v in ((0, np.full(128, 32640)), (0, np.full(127, 5)), (1, np.full(128, -16385)), (2, [5, 0, 65, 0]), (3, [0, 66, 1, 16]), (5, np.full(81, 32769)),
                 (5, np.full(70, 1)), (0, np.full(128, 0.5))):
        with pytest.raises(ValueError):
            batch.MelBank.raw(128, 64, *[v if j == i else x for j, x in enumerate(good)])
    with pytest.raises(ValueError):
        batch.MelBank.raw(128, 129, *good)


# ---------------------------------------------------------------------------------------------------------------- the check

def test_bank_check_refusals_and_the_boundaries_beside_them():
    good = list(M.raw_bound("r", 128, 128, 3, 1).record)
    N, H, B, FLAGS, WIN, CS, FIRST, COUNT, OFF, W = range(10)
    E = capi.ERR_ARG

    def rc(i=None, v=None, **kw):
        return capi.feat_bank_check(*[v if j == i else x for j, x in enumerate(good)], **kw)

    def table(i, at, v):
        a = np.array(good[i]).astype(np.int64)
        a[at] = v
        return a
    assert rc() == 0
    assert [rc(N, v) for v in (0, 64, 127, 129, 192, 4096)] == [E] * 6
    for n in (256, 512, 1024, 2048):
        assert capi.feat_bank_check(n, n, 1, 0, np.zeros(n), np.zeros(n), [0], [n // 2 + 1], [0], np.zeros(n // 2 + 1)) == 0
        assert capi.feat_bank_check(n, n, 1, 0, np.zeros(n), np.zeros(n), [1], [n // 2 + 1], [0], np.zeros(n // 2 + 2)) == E
    assert (rc(H, 0), rc(H, 1), rc(H, 128), rc(H, 129)) == (E, 0, 0, E)
    assert (rc(B, 0), rc(B, 1), rc(B, 5)) == (E, 0, E)                          # five bands: the tables have four
    assert [rc(FLAGS, f) for f in (0, 1, 2, 3, 4, 8, 1 << 31)] == [0, 0, 0, 0, E, E, E]
    assert rc(reserved=1) == E and rc(reserved=1 << 63) == E
    assert [rc(i, None) for i in (WIN, CS, FIRST, COUNT, OFF, W)] == [E] * 6
    assert (rc(WIN, table(WIN, 0, 32640)), rc(WIN, table(WIN, 127, -1)), rc(WIN, table(WIN, 127, 0)), rc(WIN, table(WIN, 64, 32767))) == (E, E, 0, E)
    assert (rc(CS, table(CS, 0, 16385)), rc(CS, table(CS, 127, -16385)), rc(CS, table(CS, 127, -16384)), rc(CS, table(CS, 3, 0))) == (E, E, 0, 0)
    assert (rc(FIRST, table(FIRST, 2, 65)), rc(FIRST, table(FIRST, 0, 65)), rc(FIRST, table(FIRST, 0, 66))) == (E, 0, E)   # a band of count 0 at bin N / 2 + 1
    assert (rc(COUNT, table(COUNT, 1, 66)), rc(COUNT, table(COUNT, 3, 66)), rc(COUNT, table(COUNT, 2, 0))) == (E, E, 0)      # refused before a weight is read
    assert (rc(W, table(W, 64, 32769)), rc(W, table(W, 64, 32768)), rc(W, table(W, 80, 65535)), rc(W, table(W, 0, 0))) == (E, 0, E, 0)
    # the 128 bands of the largest bank; a weight no band reaches is not looked at
    full = capi.feat_bank_check(2048, 1, 128, 3, np.full(2048, 32639), np.full(2048, -16384), np.zeros(128), np.full(128, 1025), np.zeros(128), np.full(1025, 32768))
    assert full == 0
    assert rc(OFF, table(OFF, 0, 10 ** 9)) == 0                                 # band 0 has no weights


# ---------------------------------------------------------------------------------------------------------------- the frame count

def test_frames_are_the_models():
    for n_fft in (128, 256, 512, 1024, 2048):
        for hop in (1, 2, 37, 160, n_fft - 1, n_fft):
            for T in (1, 2, 36, 37, 64, n_fft - 1, n_fft, n_fft + 1, n_fft + hop - 1, n_fft + hop, 2100, 6151, 16000, 2 ** 40 + 5):
                for flags in (0, 1, 2, 3):
                    assert capi.feat_frames(T, n_fft, hop, flags) == M.frames(T, n_fft, hop, flags & 1), (T, n_fft, hop, flags)
    assert capi.feat_frames(100, 128, 0, 1) == 0
    for case in M.cases():
        assert capi.feat_frames(case.frames, case.bank.n_fft, case.bank.hop, case.bank.flags) == case.F


# ---------------------------------------------------------------------------------------------------------------- the host code, sanitized

def test_layout_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "feat_layout")
    csrc = os.path.join(ROOT, "libacm_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "feat_layout.cpp"), os.path.join(csrc, "acm_feat_layout.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, "-o", exe] + src
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and "sanitize" in r.stdout and "cannot find" in r.stdout:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


# ---------------------------------------------------------------------------------------------------------------- what the cases reach

def test_the_cases_reach_what_they_claim():
    cases = M.cases()
    assert {c.frames for c in cases} == set(M.FRAMES)
    assert {c.bank.n_fft for c in cases} >= {128, 512, 2048}
    assert {c.bank.hop for c in cases} >= {1, 37, 160} and any(c.bank.hop == c.bank.n_fft for c in cases)
    assert all(c.frames == 64 for c in cases if c.bank.hop == 1)
    assert {c.F for c in cases} >= {0, 1, 16, 17, 33} and any(c.frames < c.bank.n_fft and not c.bank.center and c.F == 0 for c in cases)
    assert {c.bank.n_mels for c in cases} >= {1, 23, 80, 128}
    for center in (False, True):
        for tm in (False, True):
            assert any((c.bank.center, c.bank.time_major) == (center, tm) and c.F for c in cases), (center, tm)
    # a centred case's first and last frames reach outside the row
    assert any(c.bank.center and (c.F - 1) * c.bank.hop + c.bank.n_fft // 2 > c.frames for c in cases)
    # the raw banks: the tables at their bounds, a band of count 0, one over every bin at weight 1, one of the single bin N / 2
    raw = [c for c in cases if c.bank.name.startswith("raw")]
    assert {int(c.bank.cs[0]) for c in raw} == {M.CS_ONE, -M.CS_ONE} and all((c.bank.window == M.WINDOW_MAX).all() for c in raw)
    for c in raw:
        b = c.bank
        assert b.mel_count[0] == 0 and (b.mel_first[1], b.mel_count[1]) == (0, b.n_fft // 2 + 1) and (b.weights(1)[1] == M.W_ONE).all()
        assert (b.mel_first[2], b.mel_count[2]) == (b.n_fft // 2, 1)
    # the digits of both operands at the ends of their ranges: the windowed samples' planes over all cases, the cosines' over all banks
    ends = {"xh": set(), "xl": set(), "ch": set(), "cl": set()}
    top_a = top_e = 0
    floor_seen = zero_seen = False
    for c in cases:
        ch, cl = M.split(c.bank.cs)
        ends["ch"] |= {int(ch.min()), int(ch.max())}
        ends["cl"] |= {int(cl.min()), int(cl.max())}
        feats, detail = c.features()
        for r, d in enumerate(detail):
            if not c.F:
                continue
            assert np.abs(d["xw"]).max() <= M.WINDOW_MAX
            xh, xl = M.split(d["xw"])
            ends["xh"] |= {int(xh.min()), int(xh.max())}
            ends["xl"] |= {int(xl.min()), int(xl.max())}
            top_a = max(top_a, int(np.abs(d["A"]).max()), int(np.abs(d["Bv"]).max()))
            top_e = max([top_e] + [max(e) for e in d["E"] if e])
            row = c.rows()[0][r]
            if (row == -32768).all():
                floor_seen = True
            if not row.any():
                zero_seen = True
                assert feats[r].view(np.uint32).max() == 0              # +0.0, every bit
    assert ends["xh"] >= {-127, 127} and ends["xl"] >= {-128, 127}, ends
    assert ends["ch"] >= {-64, 64} and ends["cl"] >= {-128, 127}, ends
    assert floor_seen and zero_seen
    assert 2 ** 30 - 2 ** 23 <= top_a <= 2 ** 30, top_a
    assert 2 ** 80 <= top_e < 2 ** 89, top_e.bit_length()
    # the -32768 row under the bound banks: Re and Im at their extremes, in every whole frame
    c = next(c for c in raw if c.bank.n_fft == 2048)
    r = c.records.index(M.ident(M.FLOOR))
    d = c.features()[1][r]
    assert (d["xw"] == -M.WINDOW_MAX).all() and (d["A"] == -2 * M.WINDOW_MAX * M.CS_ONE).all() and (d["Bv"] == 2 * M.WINDOW_MAX * M.CS_ONE).all()


# ---------------------------------------------------------------------------------------------------------------- the model's meaning

def float_mel(x, rate, n_fft, win_length, hop, n_mels, f_min, f_max, center):
    """the power mel spectrogram of x (float64) the contract stands for: periodic Hann of peak 1 centred in n_fft, zero padding, HTK
    triangles without normalisation -> [n_mels, F]"""
    win = np.zeros(n_fft)
    at = (n_fft - win_length) // 2
    win[at:at + win_length] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win_length) / win_length)
    pad = n_fft // 2 if center else 0
    F = M.frames(x.size, n_fft, hop, center)
    ext = np.concatenate([np.zeros(pad), x, np.zeros(n_fft + pad)])
    fr = ext[(np.arange(F) * hop)[:, None] + np.arange(n_fft)[None, :]] * win
    power = np.abs(np.fft.rfft(fr, axis=1)) ** 2
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    corner = 700.0 * (10.0 ** ((mel(f_min) + (mel(f_max) - mel(f_min)) * np.arange(n_mels + 2) / (n_mels + 1)) / 2595.0) - 1.0)
    fk = np.arange(n_fft // 2 + 1) * float(rate) / n_fft
    W = np.stack([np.maximum(0.0, np.minimum((fk - corner[b]) / (corner[b + 1] - corner[b]), (corner[b + 2] - fk) / (corner[b + 2] - corner[b + 1])))
                  for b in range(n_mels)])
    return W @ power.T


MEANING = [((16000, 512, 512, 160, 80, 0.0, 8000.0, True), 1.04e-2),
           ((16000, 2048, 2048, 192, 128, 0.0, 8000.0, True), 1.78e-3),
           ((16000, 128, 100, 64, 23, 50.0, 7000.0, False), 1.68e-2)]


@pytest.mark.parametrize("args,measured", MEANING, ids=lambda a: "n%d_h%d_b%d" % (a[1], a[3], a[4]) if isinstance(a, tuple) else None)
def test_the_model_is_a_mel_spectrogram(args, measured):
    rate, n_fft, win_length, hop, n_mels, f_min, f_max, center = args
    rng = np.random.default_rng(0xFEA7)
    T = 16000
    x = np.rint(32768 * (0.4 * np.sin(2 * np.pi * 440.0 * np.arange(T) / rate) + 0.05 * rng.standard_normal(T))).clip(-32768, 32767).astype(np.int16)
    bank = M.design("m", rate, n_fft, win_length, hop, n_mels, f_min, f_max, M.CENTER if center else 0)
    got = M.features(x, bank).astype(np.float64)
    want = (M.WINDOW_MAX / 32768.0) ** 2 * float_mel(x / 32768.0, *args)
    assert got.shape == want.shape
    live = want > want.max() * 2.0 ** -40
    assert live.sum() > 0.9 * want.size
    err = float((np.abs(got - want)[live] / want[live]).max())
    print("n_fft %d hop %d bands %d: largest relative error %.3g over %d of %d features" % (n_fft, hop, n_mels, err, live.sum(), want.size))
    assert err <= 2 * measured, (err, measured)
