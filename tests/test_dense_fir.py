"""Dense crop batches with impulse responses without a GPU: the device-free half of acm_batch_decode_windows_overlay_fir
(libacm_amd/csrc/acm_fir_layout.cpp), the numpy model and the case list of tests/dense_fir.py, the quantiser batch.Response, and the
code the compiler makes of the kernel (libacm_amd/csrc/acm_dense_fir.hip).

  * acmk_fir_layout_visit(): every refusal with the boundary that passes beside it; the packed taps - reversed, zero-padded to the
    kernel's tap block, 16-byte aligned, each named response once; the filtered windows; the overlay's row table and list of rows
    to sum as they are uploaded, against a restatement here; the caller's own records untouched.
  * acm_dense_fir_check() and batch.Response: sum |h| on the boundary, ValueError beyond.
  * what the case list reaches, asserted on the model so that the GPU tests over the same list cannot pass vacuously.
  * the device-free half under AddressSanitizer and UBSan, as a program of its own (tests/native/fir_layout.cpp).
  * acm_dense_fir.hip compiled to gfx950 assembly: no scratch, 5120 bytes of LDS, the packed dot product with a scalar tap pair in
    the inner loop, taps through scalar loads, whole-line stores."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_fir as DF
import dense_overlay as DO
from libacm_amd import _build, batch, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = capi.OVERLAY_NONE
VISIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_size_t)
TOTALS = ("rc", "nfilt", "taps_bytes", "rows_off", "table_bytes", "nsrc", "src_arena_words", "energy_bytes", "overlay_table_bytes", "tap_block")


def visit_layout(records, nwin, row_words, responses, of_window, no_fir=False, **kw):
    """acmk_fir_layout_visit over (a, b, vol, snr, gain) records, responses [(h, d, s[, reserved])] and of_window (capi.fir_opts takes
    kw) -> (rc, tables, totals as a dict, the record table as it is after the call)"""
    L = capi.lib()
    L.acmk_fir_layout_visit.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint64, C.c_uint64, C.POINTER(capi.FirOpts), VISIT, C.c_void_p]
    n = len(records)
    table = np.zeros(max(n, 1), dtype=capi.OVERLAY_ROW_DT)
    for r, (a, b, vol, snr, gain) in enumerate(records):
        table[r] = (a, NONE if b is None else b, vol, snr, gain, 0, 0, 0)
    fir, keep = (None, None) if no_fir else capi.fir_opts(responses, of_window, **kw)
    tables = {}

    def visit(_ctx, name, data, elem_bytes, count):
        name = name.decode()
        assert name not in tables
        raw = C.string_at(data, elem_bytes * count)
        tables[name] = np.frombuffer(raw, dtype="<i2").copy() if name == "taps" else np.frombuffer(raw, dtype="<u8").reshape(count, elem_bytes // 8).copy()
    rc = L.acmk_fir_layout_visit(table.ctypes.data, n, nwin, row_words, n * row_words, C.byref(fir) if fir is not None else None, VISIT(visit), None)
    tot = dict(zip(TOTALS, tables["totals"].reshape(-1).astype(np.int64).tolist()))
    assert tot["rc"] == rc and tot["tap_block"] == DF.TB
    return rc, tables, tot, table[:n]


# ---------------------------------------------------------------------------------------------------------------- the layout

@pytest.mark.parametrize("case", DF.cases(), ids=lambda c: c.name)
def test_layout_of_the_cases(case):
    nwin, n = len(case.windows), len(case.records)
    rc, got, tot, table = visit_layout(case.records, nwin, case.row, case.responses, case.of_window)
    assert rc == 0 and list(got) == ["fir_rows", "slot", "taps", "rows", "marked", "totals"]
    # the filtered windows, ascending, each once; F of the i-th is row nwin + i
    filt = [k for k, p in enumerate(case.of_window) if p is not None]
    slot = {k: nwin + i for i, k in enumerate(filt)}
    assert got["slot"].reshape(-1).tolist() == [slot.get(k, k) for k in range(nwin)]
    # the taps: every named response once, in the order the windows come to them, reversed, zeros up to a whole tap block
    order = list(dict.fromkeys(case.of_window[k] for k in filt))
    assert DF.R_NOBODY not in order and DF.R_LONG in order and sum(case.of_window[k] == DF.R_LONG for k in filt) >= 2
    at, want = {}, []
    for p in order:
        h = case.responses[p][0]
        at[p] = len(want) // 2
        want += h[::-1].tolist() + [0] * (-h.size % DF.TB)
    assert got["taps"].tolist() == want and all(16 * (a // 4) == 4 * a for a in at.values())
    assert got["fir_rows"].astype(np.int64).tolist() == [
        [k, slot[k], at[case.of_window[k]], -(-case.responses[case.of_window[k]][0].size // DF.TB),
         case.responses[case.of_window[k]][1] - (case.responses[case.of_window[k]][0].size - 1), case.responses[case.of_window[k]][2]] for k in filt]
    # the overlay's tables as they are uploaded name the filtered rows; what the caller holds does not change
    for r, (a, b, vol, snr, gain) in enumerate(case.records):
        assert got["rows"][r].tolist() == [slot.get(a, a), NONE if b is None else slot.get(b, b), vol or 4096, snr if b is not None else 0,
                                           gain if b is not None and not snr else 0]
        assert (table["a"][r], table["b"][r]) == (a, NONE if b is None else b)
    marked = sorted({k for a, b, vol, snr, gain in case.records if b is not None and snr for k in (a, b)})
    assert got["marked"].reshape(-1).tolist() == [slot.get(k, k) for k in marked]
    assert any(k in slot for k in marked) and any(k not in slot for k in marked)
    nsrc = nwin + len(filt)
    assert (tot["nfilt"], tot["taps_bytes"], tot["rows_off"], tot["table_bytes"]) == (len(filt), 2 * len(want), 2 * len(want), 2 * len(want) + 24 * len(filt))
    assert (tot["nsrc"], tot["src_arena_words"], tot["energy_bytes"]) == (nsrc, nsrc * case.row + 64, 8 * nsrc)
    # ... and with nothing to filter the overlay's layout is the one it has without this call
    for kw in (dict(no_fir=True), dict(responses=[], of_window=None), dict(responses=case.responses, of_window=[None] * nwin)):
        rc, idle, t2, _ = visit_layout(case.records, nwin, case.row, kw.pop("responses", None), kw.pop("of_window", None), **kw)
        assert rc == 0 and (t2["nfilt"], t2["table_bytes"], t2["nsrc"], t2["src_arena_words"]) == (0, 0, nwin, nwin * case.row + 64)
        assert idle["marked"].reshape(-1).tolist() == marked and idle["rows"][:, 0].tolist() == [rec[0] for rec in case.records]
        assert t2["overlay_table_bytes"] == tot["overlay_table_bytes"] - 8 * len(filt)


def test_refusals_and_the_boundaries_beside_them():
    recs = [(0, None, 0, 0, 0), (1, 2, 4096, 65536, 0)]
    nwin, R = 3, 100
    one, edge = np.array([1], np.int16), np.full(257, 255, np.int16)
    over = edge.copy()
    over[5] = -256
    good = [(one, 0, 0), (edge, 256, 30), (np.ones(32768, np.int16), 32767, 0)]

    def rc_of(responses, of_window, **kw):
        rc, tables, tot, _ = visit_layout(recs, nwin, R, responses, of_window, **kw)
        assert rc == 0 or list(tables) == ["totals"]
        return rc
    assert rc_of(good, [0, 1, 2]) == 0
    E = capi.ERR_ARG
    # the tables
    assert rc_of(None, [0, None, None], nresp=1) == E and rc_of(good, None) == E and rc_of(None, None, nresp=0) == 0
    assert rc_of(good, [0, 1, 2], reserved=1) == E
    assert rc_of(good, [3, None, None]) == E and rc_of(good, [2, None, None]) == 0 and rc_of(good, [capi.FIR_NONE - 1, None, None]) == E
    # a response that fails the check, whether a window names it or not
    for what, bad, ok in (("no taps", (None, 0, 0), None),
                          ("delay == ntaps", (edge, 257, 0), (edge, 256, 0)),
                          ("shift 31", (edge, 0, 31), (edge, 0, 30)),
                          ("reserved", (edge, 0, 0, 1), (edge, 0, 0, 0)),
                          ("32769 taps", (np.zeros(32769, np.int16), 0, 0), (np.zeros(32768, np.int16), 0, 0)),
                          ("sum |h| 65536", (over, 0, 0), (edge, 0, 0))):
        for of in ([0, None, None], [1, None, 1]):
            assert rc_of([bad, good[1]], of) == E, what
            assert ok is None or rc_of([ok, good[1]], of) == 0, what
    # anything the overlay call refuses
    rc, tables, tot, _ = visit_layout(recs + [(3, None, 0, 0, 0)], nwin, R, good, [0, 1, 2])
    assert rc == E and list(tables) == ["totals"]
    # 2^22 taps in the responses the windows name: exactly that many pass
    full = np.ones(32768, np.int16)
    many = [(full, 0, 0)] * 129 + [(one, 0, 0)]
    wide = [(0, None, 0, 0, 0)]
    assert visit_layout(wide, 128, R, many, list(range(128)))[0] == 0
    assert visit_layout(wide, 129, R, many, list(range(128)) + [129])[0] == E
    assert visit_layout(wide, 129, R, many, list(range(128)) + [7])[0] == 0


def test_fir_check_and_the_quantiser():
    edge = [255] * 257
    assert capi.dense_fir_check([1], 0, 0) == 0 and capi.dense_fir_check(edge, 0, 30) == 0 and capi.dense_fir_check([-255] * 257, 256, 0) == 0
    assert capi.dense_fir_check(edge[:-1] + [256], 0, 0) == capi.dense_fir_check(edge[:-1] + [-256], 0, 0) == capi.ERR_ARG
    assert capi.dense_fir_check([-32768, 32767], 1, 0) == 0 and capi.dense_fir_check([-32768, 32767, 1], 1, 0) == capi.ERR_ARG
    assert capi.dense_fir_check([1], 0, 0, ntaps=0) == capi.dense_fir_check([1], 1, 0) == capi.dense_fir_check([1], 0, 31) == capi.ERR_ARG
    assert capi.dense_fir_check([1], 0, 0, reserved=1) == capi.dense_fir_check(None, 0, 0) == capi.ERR_ARG
    # Response: the largest shift at which the peak fits 16 bits and the sum fits 65535; ties to even; delay argmax |h| by default
    r = batch.Response([1.0])
    assert (r.taps.tolist(), r.delay, r.shift) == ([16384], 0, 14) and capi.dense_fir_check(r.taps, r.delay, r.shift) == 0
    r = batch.Response([0.25, -1.0, 0.5])
    assert (r.taps.tolist(), r.delay, r.shift) == ([4096, -16384, 8192], 1, 14)
    r = batch.Response([2.5, 0.5], delay=1)
    assert (r.taps.tolist(), r.delay, r.shift) == ([20480, 4096], 1, 13)
    assert batch.Response([16383.5, 0.5]).taps.tolist() == [32767, 1]
    assert batch.Response([2.5, 3.5, 0.5] + [1000.0] * 60).taps.tolist()[:3] == [2, 4, 0]                # shift 0: ties go to the even neighbour
    rng = np.random.default_rng(0xF1)
    h = rng.standard_normal(8000) * np.exp(-np.arange(8000) / 1200.0)
    h /= np.abs(h).max()
    r = batch.Response(h)
    l1 = int(np.abs(r.taps.astype(np.int64)).sum())
    assert r.delay == int(np.abs(h).argmax()) and l1 <= 65535 and np.abs(np.rint(h * 2.0 ** (r.shift + 1))).sum() > 65535
    assert np.array_equal(r.taps, np.rint(h * 2.0 ** r.shift).astype(np.int16)) and capi.dense_fir_check(r.taps, r.delay, r.shift) == 0
    # the sum on the boundary: 65535 is taken at shift 0, and nothing fits beyond
    assert batch.Response([255.0] * 257).shift == 0 and batch.Response([32767.0 / 2 ** 30]).shift == 30
    for h in ([255.0] * 256 + [256.0], [32768.0], [40000.0, 30000.0], [], [float("nan")]):
        with pytest.raises(ValueError):
            batch.Response(h)
    r = batch.Response.raw([3, -4, 5], 2, 7)
    assert (r.taps.tolist(), r.delay, r.shift, r.taps.dtype) == ([3, -4, 5], 2, 7, np.int16) and r.record[1:] == (2, 7)
    for args in (([3, -4], 2, 7), ([3, -4], 0, 31), ([255] * 256 + [256], 0, 0), ([0.5], 0, 0), ([40000], 0, 0), ([], 0, 0)):
        with pytest.raises(ValueError):
            batch.Response.raw(*args)


# ---------------------------------------------------------------------------------------------------------------- the model and the cases

def test_the_model_on_cases_by_hand():
    x = np.array([100, -200, 300, 32767, -32768], np.int16)
    y, acc = DF.fir(x, [1], 0, 0)
    assert np.array_equal(y, x) and np.array_equal(DF.fir(x, [16384], 0, 14)[0], x)
    y, acc = DF.fir(x, [2, 3], 0, 0)                                            # y[j] = 2 x[j] + 3 x[j - 1], clamped
    assert acc.tolist() == [200, -100, 0, 66434, 32765] and y.tolist() == [200, -100, 0, 32767, 32765]
    y, acc = DF.fir(x, [2, 3], 1, 0)                                            # the direct path is tap 1: y[j] = 2 x[j + 1] + 3 x[j]
    assert acc.tolist() == [-100, 0, 66434, 32765, -98304] and y.tolist()[-1] == -32768
    assert DF.fir(x, [1, 0, 0, 0, 0, 0, 0, 0, 0, 5], 9, 0)[1].tolist() == [5 * v for v in x.tolist()]
    assert DF.fir(x, [5, 0, 0, 0, 0, 0, 0, 0, 0], 8, 0)[1].tolist() == [0, 0, 0, 0, 0]      # all of it ahead of the row
    assert DF.fir(np.array([3, -3, 1, -1], np.int16), [1], 0, 1)[0].tolist() == [2, -1, 1, 0]      # (v + 1) >> 1: halves go up
    row = np.arange(12, dtype=np.int16)
    F, _ = DF.filtered(row, 2, 6, False, ([0, 1], 0, 0))                        # interleaved: a frame's delay moves two elements
    assert F.tolist() == [0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    F, _ = DF.filtered(row, 2, 6, True, ([0, 1], 0, 0))                         # planar: each plane for itself
    assert F.tolist() == [0, 0, 1, 2, 3, 4, 0, 6, 7, 8, 9, 10]


def test_case_list_reaches_what_the_kernel_can_get_wrong():
    cases = DF.cases()
    assert sorted({c.frames for c in cases}) == [1, 37, 64, 2100, 6151]
    assert {(c.channels, c.planar) for c in cases} == {(1, False), (2, False), (2, True)}
    seen = set()
    for c in cases:
        S, Fs, accs = c.sources(), c.seen(), c.accs()
        T, of, resp = c.frames, c.of_window, c.responses
        sizes = {resp[p][0].size for p in of if p is not None}
        assert sizes >= {1, 2, 3, 17, DF.TB - 1, DF.TB, DF.TB + 1, 257, 8000} and any(n > DF.STAGE and n % DF.STAGE for n in sizes)
        named = [resp[p] for p in set(of) if p is not None]
        assert {s for h, d, s in named} >= {0, 15, 30} and {0} < {d for h, d, s in named}
        assert any(d == h.size - 1 and d for h, d, s in named) and any(0 < d < h.size - 1 for h, d, s in named)
        assert all(capi.dense_fir_check(*r) == 0 for r in resp) and int(np.abs(resp[DF.R_BOUND][0].astype(np.int64)).sum()) == 65535
        # the windows: filtered and not side by side, one nobody names, one turned away, one behind its stream, one that is no ACM file
        used = {k for rec in c.records for k in rec[:2] if k is not None}
        assert of[DO.WIDE] is None and of[DF.DRY] is None and of[DO.UNUSED] is not None and DO.UNUSED not in used
        assert of[DO.AWAY] is not None and c.expect(DO.AWAY) == (0, capi.ERR_ARG) and of[DO.BEHIND] is not None and c.expect(DO.BEHIND)[0] == 0
        assert of[DO.BLOB] is not None and c.expect(DO.BLOB)[1] != 0
        for k in (DO.AWAY, DO.BEHIND, DO.BLOB):
            assert not Fs[k].any()                              # a row of zeros stays one
        snr = [(a, b) for a, b, vol, s, g in c.records if b is not None and s]
        assert any(of[a] is not None and of[b] is None for a, b in snr) and any(of[a] is None and of[b] is not None for a, b in snr)
        assert any(a == b and of[a] is not None for a, b in snr)
        # the identities are identities, and the others are not
        assert np.array_equal(Fs[DF.SAME0], S[DF.SAME0]) and np.array_equal(Fs[DF.SAME1], S[DF.SAME1]) and np.array_equal(S[DF.SAME0], S[DF.DRY])
        if T >= 37:
            for k in (DO.SPEECH, DO.STEREO, DO.UP, DO.DOWN, DO.CUT, DO.SHORT, DF.LOUD):
                assert not np.array_equal(Fs[k], S[k]), (c.name, k)
            seen.add("F differs from S")
            # the tail of a short crop rings on behind it
            assert not S[DO.SHORT][(T // 4) * (1 if c.planar else c.channels):T if c.planar else None].any()
            assert Fs[DO.SHORT][(T // 4) * (1 if c.planar else c.channels):T if c.planar else None].any(), c.name
        for k, per_channel in accs.items():
            for acc in per_channel:
                h, d, s = resp[of[k]]
                assert np.abs(acc).max(initial=0) <= 65535 * 32768
                v = (acc + ((1 << (s - 1)) if s else 0)) >> s
                seen |= {"acc beyond 2^30"} if (np.abs(acc) >= 2 ** 30).any() else set()
                seen |= {"clamped at +32767"} if (v > 32767).any() else set()
                seen |= {"clamped at -32768"} if (v < -32768).any() else set()
                seen |= {"a negative sum rounded"} if s and ((acc < 0) & (acc % (1 << s) != 0)).any() else set()
        if T >= 2100:
            # the sign-matched response meets the samples it was made from
            x = DF.channel(S[DF.LOUD], c.channels, T, c.planar, 0)
            h, j0 = DF.sign_matched(x)
            assert np.array_equal(h, resp[DF.R_BOUND][0]) and j0 >= 256
            assert accs[DF.LOUD][0][j0] == 255 * int(np.abs(x[j0 - 256:j0 + 1].astype(np.int64)).sum()) >= 2 ** 30
        if T == 6151:
            # a tile reads inputs of the tile in front of it and of the one behind it: silence there changes its outputs
            for k, edge in ((DO.UP, 2048), (DO.SPEECH, 4096)):
                h, d, s = resp[of[k]]
                x = DF.channel(S[k], c.channels, T, c.planar, 0).copy()
                y = DF.fir(x, h, d, s)[0]
                front, behind = x.copy(), x.copy()
                front[:edge - 8] = 0
                behind[edge + 2048:] = 0
                for what, z in (("inputs from the tile in front", front), ("inputs from the tile behind", behind)):
                    if not np.array_equal(DF.fir(z, h, d, s)[0][edge:edge + 2040], y[edge:edge + 2040]):
                        seen.add(what)
            # the long response has taps on both sides of the row at once: outputs near either end use fewer than all taps, on both sides
            h, d, s = resp[DF.R_LONG]
            assert h.size > T and 0 < d < h.size - 1 and d < T and h.size - 1 - d < T
            seen.add("taps from both sides of [0, T)")
        if T == 37:
            h, d, s = resp[DF.R_LONG]
            assert h.size - 1 - d > T and d > T                 # every output of the row reads beyond both ends
    want = {"F differs from S", "acc beyond 2^30", "clamped at +32767", "clamped at -32768", "a negative sum rounded",
            "inputs from the tile in front", "inputs from the tile behind", "taps from both sides of [0, T)"}
    assert seen >= want, want - seen


# ---------------------------------------------------------------------------------------------------------------- the host code, sanitized

def test_layout_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "fir_layout")
    csrc = os.path.join(ROOT, "libacm_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "fir_layout.cpp"), os.path.join(csrc, "acm_fir_layout.cpp"), os.path.join(csrc, "acm_overlay_layout.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, "-o", exe] + src
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and "sanitize" in r.stdout and "cannot find" in r.stdout:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


# ---------------------------------------------------------------------------------------------------------------- the kernel's code

@pytest.fixture(scope="module")
def kernel_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "acm_dense_fir.s"
    cmd = [_build.HIPCC, "-O3", "-std=c++17", "--offload-arch=" + _build.GFX, "-I", _build.INC, "-I", _build.CSRC,
           "--cuda-device-only", "-S", "-o", str(out), os.path.join(_build.CSRC, "acm_dense_fir.hip")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return out.read_text()


def test_kernel_code(kernel_asm):
    """both builds (a channel's frames one element apart, and two): no private segment; LDS is the stage alone - a tile and eight tap
    blocks of int16, 5120 bytes, a thirty-second of a CU's; the inner loop is 8 packed dot products per tap pair with the pair in a
    scalar register, the pairs come through scalar loads, its input through ds_read_b128; no flat, buffer or scratch access; whole
    lines are stored where a channel is contiguous"""
    bodies = {}
    for m in re.finditer(r"^(_ZN\S*acm_dense_fir\S*):", kernel_asm, re.M):
        bodies[m.group(1)] = kernel_asm[m.end():kernel_asm.index(".Lfunc_end", m.end())]
    assert len(bodies) == 2, sorted(bodies)
    for name, body in bodies.items():
        ops = re.findall(r"^\s+((?:global|flat|scratch|buffer|ds)_\w+)", body, re.M)
        assert not [o for o in ops if o.startswith(("flat_", "scratch_", "buffer_", "global_atomic"))], (name, sorted(set(ops)))
        meta = re.search(r"\.name:\s+%s\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)" % re.escape(name), kernel_asm)
        assert meta and int(meta.group(1)) == 0, name
        desc = kernel_asm[kernel_asm.index(".amdhsa_kernel " + name):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)\b", desc).group(1))
        assert lds == 2 * (2048 + DF.STAGE) == 5120 and 4 * lds <= 160 * 1024, (name, lds)
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)\b", desc).group(1))
        assert vgprs <= 128, (name, vgprs)                      # four workgroups of four wavefronts a CU: 128 registers a lane
        # the inner loop: the innermost loop that holds the dot products, from its label to its backward branch
        dots = [m.start() for m in re.finditer(r"^\s+v_dot2c?_i32_i16", body, re.M)]
        assert len(dots) == 8 * DF.TB // 2, (name, len(dots))
        head = body.rindex("\n.LBB", 0, dots[0])
        label = re.match(r"\n(\.LBB\w+):", body[head:]).group(1)
        loop = body[head:body.index("s_cbranch", dots[-1])]
        assert re.search(r"s_cbranch_\w+ %s\b" % re.escape(label), body[dots[-1]:dots[-1] + 2000]), name
        scalar_taps = re.findall(r"^\s+v_dot2c?_i32_i16\w* v\d+, (s\d+), v\d+", loop, re.M)
        assert len(scalar_taps) == len(dots) and len(set(scalar_taps)) == DF.TB // 2, (name, len(scalar_taps), len(set(scalar_taps)))
        assert sum(int(n) for n in re.findall(r"^\s+s_load_dwordx(\d+)", loop, re.M)) == DF.TB // 2, name
        assert loop.count("ds_read_b128") == DF.TB // 8 + 1 and not re.search(r"^\s+(global_load|ds_write|s_barrier)", loop, re.M), name
        other = len(re.findall(r"^\s+v_\w+", loop, re.M)) - len(dots)
        assert other <= 48, (name, other)                       # an alignment per dword of input and the loop's own few
        assert ("global_store_dwordx4" in ops) == ("ILi1E" in name), (name, sorted(set(ops)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(_build.CSRC, "acm_dense_fir.hip")).read(), flags=re.S)
    assert src.count("dense_geo(") == 1 and "acm_cap_value" not in src and not re.search(r"\b(nwork|units|grid) = ", src)
