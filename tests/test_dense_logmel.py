"""Log-mel features from dense crop batches without a GPU: the device-free half of acm_batch_decode_windows_logmel
(libacm_amd/csrc/acm_feat_layout.h and .cpp), the numpy model and the case list of tests/dense_logmel.py.

  * the integer logarithm over all 2^23 mantissas: x stays in [2^23, 2^24), frac is monotone, frac(2^23) = 0, frac(2^24 - 1) = 65535
    and 0 <= 65536 * log2(m / 2^23) - frac(m) < 1.02 (1.009 measured: the sixteen truncations of x each lose a little, downwards).
  * the scale: V within half a unit of offset + L * mul / 2^24.
  * acm_feat_log_check(): every refusal with the boundary that passes beside it, against the model's own check.
  * the device-free half under AddressSanitizer and UBSan, as a program of its own (tests/native/feat_log.cpp): acm_feat_log_q16
    against 128 bits.
  * batch.LogScale: the fields of the four kinds and of whisper(), by hand.
  * what the case list reaches, asserted on the model so that the GPU tests over the same list cannot pass vacuously.

Every test here needs acm_feat_log_check or batch.LogScale, which the library did not have before."""
import math
import os
import subprocess

import numpy as np
import pytest

import dense_feat as M
import dense_logmel as G
from libacm_amd import batch, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the logarithm

def test_every_mantissa():
    assert capi.feat_log_check(M.raw_bound("r", 128, 128, 3, 1).record, G.LOG2.record) == 0     # (the entry point these tests are about)
    m = np.arange(1 << 23, 1 << 24, dtype=np.uint64)
    f, inside = G.frac(m)
    assert inside
    assert int(f[0]) == 0 and int(f[-1]) == 65535
    assert (np.diff(f.astype(np.int64)) >= 0).all()
    err = 65536.0 * np.log2(m.astype(np.float64) / float(1 << 23)) - f.astype(np.float64)
    print("65536 * log2(m / 2^23) - frac(m): %.6f .. %.6f over %d mantissas" % (err.min(), err.max(), m.size))
    assert err.min() >= 0 and err.max() < 1.02


def test_log_of_single_values():
    # powers of two are exact; L is log2 of the linear feature, in Q16
    for n in (7, 9, 11):
        for p in (0, 1, 23, 24, 40, 64, 88):
            assert int(G.log_q16([1 << p], n, -G.FLOOR_MAX)[0]) == (p - (75 - 2 * n)) * 65536
        E = [3, 5, (1 << 64) + 12345, (1 << 88) - 1, 1000003]
        L = G.log_q16(E, n, -G.FLOOR_MAX)
        for e, l in zip(E, L):
            y = M.trunc24(e, n)
            assert 0 <= 65536 * math.log2(float(y)) - int(l) < 1.02, (e, n)
    assert G.log_q16([0, 1, 0], 9, -7).tolist() == [-7, -7, -7] and G.log_q16([0, 1 << 70], 9, 5).tolist() == [5, 13 * 65536]


def test_scale_identity():
    rng = np.random.default_rng(0x106)
    L = np.concatenate([rng.integers(-G.FLOOR_MAX, 62 * 65536, 20000), [0, 1, -1, -G.FLOOR_MAX, 62 * 65536, G.FLOOR_MAX]]).astype(np.int64)
    for s in G.SCALES + (G.DB30, G.Scale("odd", 0, 0, 1, 77, 0), G.Scale("half", 0, 0, 1 << 23, -1, 0)):
        V = G.scaled(L, s)
        exact = L.astype(np.float64) * s.mul_q24 / float(1 << 24)              # below 2^53: L * mul is exact in a double
        assert np.abs((V - s.offset_q16) - exact).max() <= 0.5, s.name
        assert np.abs(V).max() < 1 << 24 or not G.check(s.record)
        f = (V.astype(np.float64) / 65536.0).astype(np.float32)
        assert (f.astype(np.float64) * 65536.0 == V).all()                      # the float32 is exact


# ---------------------------------------------------------------------------------------------------------------- the check

def test_log_check_refusals_and_the_boundaries_beside_them():
    bank = M.raw_bound("r", 128, 128, 3, 1).record
    E = capi.ERR_ARG
    FLAGS, FLOOR, MUL, OFF, TOP = range(5)
    good = list(G.WHISPER.record)

    def rc(i=None, v=None, base=good, **kw):
        rec = [v if j == i else x for j, x in enumerate(base)]
        got = capi.feat_log_check(bank, dict(zip(("flags", "floor_q16", "mul_q24", "offset_q16", "top_q16"), rec), **kw))
        assert (got == 0) == G.check(tuple(rec), kw.get("reserved", 0)), (rec, kw, got)
        return got
    assert rc() == 0
    assert capi.feat_log_check(bank, None) == E
    assert capi.feat_log_check(bank[:3] + (4,) + bank[4:], good) == E           # a bank the features call refuses
    assert capi.feat_log_check(dict(zip(("n_fft", "hop", "n_mels", "flags", "window", "cs", "mel_first", "mel_count", "mel_off", "mel_w"), bank), reserved=1), good) == E
    assert [rc(FLAGS, f) for f in (1, 2, 3, 1 << 31)] == [0, E, E, E]
    assert rc(reserved=1) == E and rc(reserved=1 << 31) == E
    notop = [0] + good[1:4] + [0]
    assert (rc(base=notop), rc(TOP, 1, base=notop), rc(TOP, G.TOP_MAX, base=notop)) == (0, E, E)               # a top without the flag
    assert (rc(TOP, 0), rc(TOP, G.TOP_MAX), rc(TOP, G.TOP_MAX + 1), rc(TOP, 2 ** 32 - 1)) == (0, 0, E, E)
    assert (rc(FLOOR, -G.FLOOR_MAX), rc(FLOOR, -G.FLOOR_MAX - 1), rc(FLOOR, G.FLOOR_MAX), rc(FLOOR, G.FLOOR_MAX + 1), rc(FLOOR, -2 ** 31)) == (0, E, 0, E, E)
    assert (rc(MUL, 0), rc(MUL, 1), rc(MUL, G.MUL_MAX), rc(MUL, G.MUL_MAX + 1)) == (E, 0, E, E)                 # 2^28 is in range and past the bound
    # the bound, Lb = 62 * 65536 at mul 2^24: |offset| up to 2^24 - Lb - 2
    one = [0, -2177059, 1 << 24, 0, 0]
    edge = (1 << 24) - 62 * 65536 - 2
    assert (rc(OFF, edge, base=one), rc(OFF, edge + 1, base=one), rc(OFF, -edge, base=one), rc(OFF, -edge - 1, base=one)) == (0, E, 0, E)
    assert (rc(OFF, -2 ** 31, base=one), rc(OFF, 2 ** 31 - 1, base=one)) == (E, E)
    # ... and with a floor beyond 62: Lb = 64 * 65536
    low = [0, -G.FLOOR_MAX, 1 << 24, 0, 0]
    edge = (1 << 24) - 64 * 65536 - 2
    assert (rc(OFF, edge, base=low), rc(OFF, edge + 1, base=low)) == (0, E)
    high = [0, G.FLOOR_MAX, 1 << 24, 0, 0]
    assert (rc(OFF, edge, base=high), rc(OFF, edge + 1, base=high)) == (0, E)
    assert (rc(MUL, (1 << 26) - 17, base=low), rc(MUL, 1 << 26, base=low)) == (0, E)
    # every scale of the case list is one the call takes
    for s in G.SCALES + (G.DB30,):
        assert rc(base=list(s.record)) == 0, s.name


# ---------------------------------------------------------------------------------------------------------------- the host code, sanitized

def test_log_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "feat_log")
    csrc = os.path.join(ROOT, "libacm_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "feat_log.cpp"), os.path.join(csrc, "acm_feat_layout.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, "-o", exe] + src
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


# ---------------------------------------------------------------------------------------------------------------- python

def test_log_scale_fields():
    # (flags, floor_q16, mul_q24, offset_q16, top_q16), worked out by hand in tests/dense_logmel.py
    assert batch.LogScale("log2", floor=2.0 ** -64).record == G.LOG2.record
    assert batch.LogScale().record == batch.LogScale("ln").record == G.LN.record
    assert batch.LogScale("db", top=80.0).record == G.DB80.record
    assert batch.LogScale.whisper().record == G.WHISPER.record
    assert batch.LogScale("log10").record == (0, -2177059, 5050445, 0, 0)
    assert batch.LogScale("log10", floor=1.0, top=0.0, post_mul=2.0, post_add=-0.5).record == (1, 0, 10100891, -32768, 0)
    assert batch.LogScale("db", top=30.0).top_q16 == G.DB30.top_q16
    w = batch.LogScale.whisper()
    assert (w.kind, w.flags, w.floor_q16, w.mul_q24, w.offset_q16, w.top_q16) == ("log10",) + G.WHISPER.record
    r = batch.LogScale.raw(-5, 77, -3, 9)
    assert r.record == (1, -5, 77, -3, 9) and batch.LogScale.raw(-5).record == (0, -5, 1 << 24, 0, 0)
    for bad in (dict(kind="log3"), dict(floor=0.0), dict(floor=-1.0), dict(top=-1.0)):
        with pytest.raises(ValueError):
            batch.LogScale(**bad)
    with pytest.raises(ValueError):
        batch.LogScale.raw(-2 ** 31 - 1)
    # a scale the check refuses is the decoder's ValueError: the check is the library's
    bank = M.raw_bound("r", 128, 128, 3, 1).record
    assert capi.feat_log_check(bank, batch.LogScale("db", post_mul=2.0).record) == capi.ERR_ARG
    assert capi.feat_log_check(bank, batch.LogScale.whisper().record) == 0


# ---------------------------------------------------------------------------------------------------------------- what the cases reach

def test_the_cases_reach_what_they_claim():
    cases = G.cases()
    assert [c.name for c in cases[:20]] == ["%s_%s" % (n, s.name) for n in G.BASE for s in G.SCALES]
    assert len({c.name for c in cases}) == len(cases)
    reached = dict.fromkeys(("floor_some", "all_floor", "top_some", "two_maxima", "last_tile", "last_tile_of_many", "second_slot", "both_signs"), False)
    for c in cases:
        out, detail = c.logmel()
        bank, F, s = c.case.bank, c.case.F, c.scale
        assert out.shape == c.case.features()[0].shape and out.dtype == np.float32
        if not F:
            continue
        tiles = -(-F // M.TILE)
        tops = set()
        for r, d in enumerate(detail):
            L, Lc = d["L"], d["Lc"]                                                  # [B, F]
            at_floor = L == s.floor_q16
            lin = c.case.features()[0][r]
            lin = lin.T if bank.time_major else lin
            # the floor is active where the linear feature is 0 or its logarithm no more than the floor
            true = np.where(lin > 0, 65536.0 * np.log2(np.where(lin > 0, lin, 1).astype(np.float64)), -np.inf)
            assert (L >= s.floor_q16).all() and (true[at_floor] < s.floor_q16 + 1.02).all() and (true[~at_floor] > s.floor_q16).all()
            reached["floor_some"] |= bool(at_floor.any() and not at_floor.all())
            if not c.case.rows()[0][r].any():
                assert at_floor.all() and d["M"] == s.floor_q16
                reached["all_floor"] = True
            reached["both_signs"] |= bool((L < 0).any() and (L > 0).any())
            if not s.top:
                assert (Lc == L).all()
                continue
            tops.add(d["M"])
            share = float((Lc != L).mean())
            reached["top_some"] |= 0.01 <= share <= 0.99
            where = np.argwhere(L == d["M"])
            # every place of the maximum in the row's last tile, which is a partial one: the table needs that tile's wavefronts
            if F % M.TILE and (where[:, 1] >= (tiles - 1) * M.TILE).all():
                reached["last_tile"] = True
                reached["last_tile_of_many"] |= tiles > 1
            reached["second_slot"] |= bool((where[:, 0] >= 16).all())
        reached["two_maxima"] |= len(tops) > 1
    assert all(reached.values()), reached
    # the quiet case's maxima lie far below the loud one's, row by row: a table that was not reset shows
    loud, quiet = G.pick("loud_t2100_d128_hN_b23_db_top30"), G.pick("quiet_t2100_d128_hN_b23_db_top30")
    for a, b in zip(loud.logmel()[1], quiet.logmel()[1]):
        assert a["M"] - b["M"] > G.DB30.top_q16
        assert (np.maximum(b["L"], a["M"] - G.DB30.top_q16) != b["Lc"]).any()
