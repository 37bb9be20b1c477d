"""Dense crop batches with an overlay without a GPU: the device-free half of acm_batch_decode_windows_overlay
(libacm_amd/csrc/acm_overlay_layout.cpp), the numpy model and the case list of tests/dense_overlay.py, and the code the compiler makes
of the kernels (libacm_amd/csrc/acm_dense_overlay.hip).

  * acm_dense_overlay_gain() against the integer model, on the extremes and on 20 000 seeded draws; the model against a binary-search
    restatement that divides nothing.
  * acmk_overlay_layout_visit(): every refusal of the row table, the kernel's records, the source rows that get an energy, the
    sizes of the source arena and of the tables.
  * the model's identity row, and what the case list reaches - asserted here so that the GPU tests over the same list cannot pass
    vacuously.
  * the python helpers: snr_q16, gain_q12, Overlay.
  * the device-free half under AddressSanitizer and UBSan, as a program of its own (tests/native/overlay_layout.cpp).
  * acm_dense_overlay.hip compiled to gfx950 assembly: no scratch in any build, LDS in the reduction alone, one 64-bit atomic."""
import ctypes as C
import os
import re
import subprocess
from math import isqrt

import numpy as np
import pytest

import dense_overlay as DO
from libacm_amd import _build, batch, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = capi.OVERLAY_NONE
VISIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_size_t)
TOTALS = ("rc", "row_words", "out_words", "src_arena_words", "upload_bytes", "energy_off", "energy_bytes", "result_off", "result_bytes", "table_bytes")


# ---------------------------------------------------------------------------------------------------------------- the gain

def search(ea, eb, snr):
    """the contract's g without a division: the largest g <= G_MAX with g^2 * D <= Ea << 40"""
    D, N = eb * snr, ea << 40
    if D == 0:
        return 0
    lo, hi = 0, DO.G_MAX
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if mid * mid * D <= N else (lo, mid - 1)
    return lo


EXTREMES = [(0, 0, 0), (0, 5, 65536), (5, 0, 65536), (5, 5, 0), (1000, 1000, 65536), (1000, 1000, 1), (1000, 1000, 2 ** 32 - 1),
            (2 ** 54 - 1, 2 ** 54 - 1, 2 ** 32 - 1), (2 ** 54 - 1, 1, 1), (1, 2 ** 54 - 1, 2 ** 32 - 1), (1, 2 ** 54 - 1, 1), (64, 1, 65536),
            (63, 1, 65536), (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 32 - 1), (2 ** 64 - 1, 1, 1), (1, 2 ** 64 - 1, 2 ** 32 - 1), (1, 1, 2 ** 32 - 1),
            (1 << 30, 1 << 30, 65537), ((1 << 30) * (2 ** 24 - 1), 1, 2 ** 32 - 1)]


def test_gain_on_the_extremes():
    for ea, eb, snr in EXTREMES:
        assert capi.dense_overlay_gain(ea, eb, snr) == DO.gain(ea, eb, snr) == search(ea, eb, snr), (ea, eb, snr)
    assert [DO.gain(*e) for e in EXTREMES[:7]] == [0, 0, 0, 0, 4096, 32768, 16]
    assert DO.gain(63, 1, 65536) == isqrt(63 << 24) == 32510


def test_gain_on_seeded_draws():
    rng = np.random.default_rng(0x0E41A7)
    n = 20000
    # energies of every size below 2^54, ratios of every size in 32 bits
    ea = rng.integers(0, 2 ** 54, n, dtype=np.uint64) >> rng.integers(0, 54, n).astype(np.uint64)
    eb = rng.integers(0, 2 ** 54, n, dtype=np.uint64) >> rng.integers(0, 54, n).astype(np.uint64)
    snr = rng.integers(1, 2 ** 32, n, dtype=np.uint64) >> rng.integers(0, 32, n).astype(np.uint64)
    seen = set()
    for a, b, s in zip(ea.tolist(), eb.tolist(), snr.tolist()):
        want = DO.gain(a, b, s)
        assert capi.dense_overlay_gain(a, b, s) == want == search(a, b, s), (a, b, s)
        seen.add("zero" if want == 0 else "top" if want == DO.G_MAX else "inside")
    assert seen == {"zero", "top", "inside"}


# ---------------------------------------------------------------------------------------------------------------- the layout

def visit_layout(rows, nwin, row_words, d_pcm_words=None, nrows=None):
    """acmk_overlay_layout_visit over (a, b, vol, snr, gain[, reserved]) rows (b None: ACM_OVERLAY_NONE; rows None: no table) ->
    (rc, tables as uint64 arrays, the totals as a dict)"""
    L = capi.lib()
    L.acmk_overlay_layout_visit.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint64, C.c_uint64, VISIT, C.c_void_p]
    n = len(rows) if rows is not None else 0
    table = (capi.OverlayRow * max(n, 1))()
    for r in range(n):
        a, b, vol, snr, gain = rows[r][:5]
        table[r] = capi.OverlayRow(a, NONE if b is None else b, vol, snr, gain, rows[r][5] if len(rows[r]) > 5 else 0, 0, 0)
    n = n if nrows is None else nrows
    tables = {}

    def visit(_ctx, name, data, elem_bytes, count):
        assert name.decode() not in tables and elem_bytes % 8 == 0
        tables[name.decode()] = np.frombuffer(C.string_at(data, elem_bytes * count), dtype="<u8").reshape(count, elem_bytes // 8).copy()
    rc = L.acmk_overlay_layout_visit(table if rows is not None else None, n, nwin, row_words, n * row_words if d_pcm_words is None else d_pcm_words,
                                     VISIT(visit), None)
    tot = dict(zip(TOTALS, tables["totals"].reshape(-1).astype(np.int64).tolist()))
    assert tot["rc"] == rc
    return rc, tables, tot


@pytest.mark.parametrize("case", DO.cases(), ids=lambda c: c.name)
def test_layout_of_the_cases(case):
    nwin, n = len(case.windows), len(case.records)
    rc, got, tot = visit_layout(case.records, nwin, case.row)
    assert rc == 0 and list(got) == ["rows", "marked", "totals"]
    for r, (a, b, vol, snr, gain) in enumerate(case.records):
        assert got["rows"][r].tolist() == [a, NONE if b is None else b, vol or 4096, snr if b is not None else 0, gain if b is not None and not snr else 0]
    # a source row is summed once however many rows name it, and only if a row in SNR mode does
    marked = sorted({k for a, b, vol, snr, gain in case.records if b is not None and snr for k in (a, b)})
    assert got["marked"].reshape(-1).tolist() == marked and DO.UNUSED not in marked and DO.UP in marked
    assert (tot["row_words"], tot["out_words"], tot["src_arena_words"]) == (case.row, n * case.row, nwin * case.row + 64)
    up = -(-(24 * n + 4 * len(marked)) // 8) * 8
    assert (tot["upload_bytes"], tot["energy_off"], tot["energy_bytes"], tot["result_off"], tot["result_bytes"], tot["table_bytes"]) == \
        (up, up, 8 * nwin, up + 8 * nwin, 24 * n, up + 8 * nwin + 24 * n)


def test_refusals_of_the_row_table():
    good = [(0, None, 0, 0, 0), (1, 2, 4096, 65536, 0), (2, 0, 65535, 0, 32768), (3, 3, 1, 2 ** 32 - 1, 0)]
    nwin, R = 4, 100
    assert visit_layout(good, nwin, R)[0] == 0
    for what, rows, kw in (("no table for rows", None, dict(nrows=2, d_pcm_words=2 * R)),
                           ("a == nwin", good + [(4, None, 0, 0, 0)], {}),
                           ("a is ACM_OVERLAY_NONE", good + [(NONE, None, 0, 0, 0)], {}),
                           ("b == nwin", good + [(0, 4, 0, 0, 0)], {}),
                           ("b one below ACM_OVERLAY_NONE", good + [(0, NONE - 1, 0, 65536, 0)], {}),
                           ("reserved", good + [(0, 1, 0, 65536, 0, 1)], {}),
                           ("reserved without b", good + [(0, None, 0, 0, 0, 7)], {}),
                           ("an absolute gain above G_MAX", good + [(0, 1, 0, 0, 32769)], {}),
                           ("a volume beyond 16 bits", good + [(0, 1, 65536, 65536, 0)], {}),
                           ("a tensor one element short", good, dict(d_pcm_words=4 * R - 1))):
        rc, tables, tot = visit_layout(rows, nwin, R, **kw)
        assert rc == capi.ERR_ARG and list(tables) == ["totals"], what
    # a row of 2^24 elements and more
    assert visit_layout(good, nwin, 2 ** 24, d_pcm_words=2 ** 64 - 1)[0] == capi.ERR_ARG
    assert visit_layout(good, nwin, 2 ** 24 - 1)[0] == 0
    # accepted next to them: `gain` is read in absolute mode alone, room to spare, no rows at all
    assert visit_layout(good + [(0, 1, 0, 65536, 40000), (0, None, 0, 0, 40000)], nwin, R)[0] == 0
    assert visit_layout(good, nwin, R, d_pcm_words=4 * R + 1)[0] == 0
    rc, tables, tot = visit_layout([], nwin, R)
    assert rc == 0 and tables["rows"].size == 0 and tables["marked"].size == 0 and tot["table_bytes"] == 8 * nwin and tot["out_words"] == 0
    rc, tables, tot = visit_layout(None, 0, R)
    assert rc == 0 and tot["table_bytes"] == 0 and tot["src_arena_words"] == 64


# ---------------------------------------------------------------------------------------------------------------- the model and the cases

def test_the_identity_row_is_its_source():
    for case in DO.cases():
        src = case.sources()
        out, gains = case.rows()
        ident = [(r, rec[0]) for r, rec in enumerate(case.records) if rec[1] is None and rec[2] in (0, 4096)]
        assert len(ident) >= len(case.windows) - 1
        for r, a in ident:
            assert np.array_equal(out[r], src[a]) and gains[r] == (0, 0, 0), (case.name, r)
    x = np.arange(-32768, 32768, dtype=np.int16)
    assert np.array_equal(DO.combine(x, x, 0, 4096), x) and np.array_equal(DO.combine(x, x[::-1], 0, 0), x)


def test_case_list_reaches_what_the_kernels_can_get_wrong():
    cases = DO.cases()
    assert sorted({c.frames for c in cases}) == sorted(DO.FRAMES) == [1, 37, 64, 2100, 6151]
    assert {(c.channels, c.planar) for c in cases} == {(1, False), (2, False), (2, True)}
    seen = set()
    for c in cases:
        src = c.sources()
        out, gains = c.rows()
        recs = c.records
        # the rows the issue names
        assert {rec[2] for rec in recs if rec[1] is None} >= {4096, 2048, 65535}
        assert any(rec[0] == rec[1] for rec in recs)
        used = [rec[0] for rec in recs] + [rec[1] for rec in recs if rec[1] is not None]
        assert max(sum(1 for rec in recs if rec[1] == k) for k in range(len(src))) >= 4 and DO.UNUSED not in used
        order = [rec[0] for rec in recs]
        assert any(order[i] > order[i + 1] > order[i + 2] for i in range(len(order) - 2))
        assert {rec[3] for rec in recs} >= {1, 2 ** 32 - 1} and {rec[4] for rec in recs if rec[1] is not None and not rec[3]} >= {0, 32768}
        assert c.expect(DO.AWAY) == (0, capi.ERR_ARG) and c.expect(DO.BEHIND)[0] == 0 and not src[DO.AWAY].any() and not src[DO.BEHIND].any()
        if c.frames >= 37:
            assert all(src[k].any() for k in range(len(src)) if k not in (DO.AWAY, DO.BEHIND, DO.BLOB)), c.name
        for r, (rec, (g, ea, eb)) in enumerate(zip(recs, gains)):
            a, b, vol, snr, gain = rec
            if b is not None and snr:
                assert (ea, eb) == (DO.energy(src[a]), DO.energy(src[b])) and g == DO.gain(ea, eb, snr)
                seen.add("g 0 by Eb == 0" if g == 0 and eb == 0 and ea else "g 0 by Ea == 0" if g == 0 and ea == 0 and eb else
                         "g inside" if 0 < g < DO.G_MAX else "g at G_MAX" if g == DO.G_MAX else "g 0")
            hi, lo = int((out[r] == 32767).sum()), int((out[r] == -32768).sum())
            B = src[b] if b is not None else np.zeros_like(src[a])
            p = DO.products(src[a], B, g, vol)
            clamped = int(((p >> 24) > 32767).sum() + ((p >> 24) < -32768).sum())
            if clamped:
                seen |= {"clamped at +32767"} if ((p >> 24) > 32767).any() else set()
                seen |= {"clamped at -32768"} if ((p >> 24) < -32768).any() else set()
                assert 2 * clamped < out[r].size and hi + lo >= clamped, (c.name, r, clamped)
            if ((p < 0) & (p % (1 << 24) == 0)).any():
                seen.add("a negative exact multiple of 2^24")
                if vol == 2048 and b is None:
                    seen.add("... by vol 2048 over an odd negative sample")
        if c.frames == 6151 and c.channels == 1:
            # A, B and the output at three different alignments in one row: row k lies k * R samples into its arena
            assert any(len({(a * c.row) % 8, (b * c.row) % 8, (r * c.row) % 8}) == 3 for r, (a, b, *_) in enumerate(recs) if b is not None)
            seen.add("three alignments")
        if c.row > 3 * 2048:
            seen.add("an energy summed by four workgroups" if -(-c.row // 2048) == 4 else "... by more")
    want = {"g 0 by Eb == 0", "g 0 by Ea == 0", "g inside", "g at G_MAX", "clamped at +32767", "clamped at -32768",
            "a negative exact multiple of 2^24", "... by vol 2048 over an odd negative sample", "three alignments",
            "an energy summed by four workgroups"}
    assert seen >= want, want - seen


def test_python_helpers():
    assert [batch.snr_q16(db) for db in (0, 10, -10, 20, -60, 60)] == [65536, 655360, 6554, 6553600, 1, 2 ** 32 - 1]
    assert [batch.gain_q12(db) for db in (0, -6, 6, 20, -200)] == [4096, 2053, 8173, 32768, 0]
    assert [batch.gain_q12(db, 1, 65535) for db in (0, 30, -200)] == [4096, 65535, 1]
    assert batch.Overlay(3).record() == (3, None, 4096, 0, 0)
    assert batch.Overlay(3, b=9, snr_db=10).record() == (3, 9, 4096, 655360, 0)
    assert batch.Overlay(3, b=9, gain_db=-6, vol_db=6).record() == (3, 9, 8173, 0, 2053)
    for kw in (dict(b=1), dict(b=1, snr_db=3, gain_db=3), dict(snr_db=3), dict(gain_db=0)):
        with pytest.raises(ValueError):
            batch.Overlay(0, **kw)


# ---------------------------------------------------------------------------------------------------------------- the host code, sanitized

def test_layout_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "overlay_layout")
    csrc = os.path.join(ROOT, "libacm_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "overlay_layout.cpp"), os.path.join(csrc, "acm_overlay_layout.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, "-o", exe] + src
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and "sanitize" in r.stdout and "cannot find" in r.stdout:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


# ---------------------------------------------------------------------------------------------------------------- the kernels' code

@pytest.fixture(scope="module")
def kernel_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "acm_dense_overlay.s"
    cmd = [_build.HIPCC, "-O3", "-std=c++17", "--offload-arch=" + _build.GFX, "-I", _build.INC, "-I", _build.CSRC,
           "--cuda-device-only", "-S", "-o", str(out), os.path.join(_build.CSRC, "acm_dense_overlay.hip")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return out.read_text()


def test_kernels_have_no_scratch(kernel_asm):
    """the energy kernel, the gain kernel and both builds of the combine kernel: no private segment, LDS in the reduction alone (32
    bytes), 16-byte global loads, whole-line stores in the combine kernel, one 64-bit atomic add in the energy kernel, no flat, buffer
    or scratch access"""
    bodies = {}
    for m in re.finditer(r"^(_ZN\S*acm_dense_(?:energy|gains|overlay)\S*):", kernel_asm, re.M):
        bodies[m.group(1)] = kernel_asm[m.end():kernel_asm.index(".Lfunc_end", m.end())]
    assert len(bodies) == 4 and sum("energy" in name for name in bodies) == 1 and sum("gains" in name for name in bodies) == 1, sorted(bodies)
    for name, body in bodies.items():
        ops = re.findall(r"^\s+((?:global|flat|scratch|buffer|ds)_\w+)", body, re.M)
        assert not [o for o in ops if o.startswith(("flat_", "scratch_", "buffer_"))], (name, sorted(set(ops)))
        assert "gains" in name or "global_load_dwordx4" in ops, (name, sorted(set(ops)))
        meta = re.search(r"\.name:\s+%s\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)" % re.escape(name), kernel_asm)
        assert meta and int(meta.group(1)) == 0, name
        desc = kernel_asm[kernel_asm.index(".amdhsa_kernel " + name):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)\b", desc).group(1))
        if "energy" in name:
            assert lds == 32 and ops.count("global_atomic_add_x2") == 1 and not [o for o in ops if o.startswith("global_store")], (name, sorted(set(ops)))
        elif "gains" in name:
            assert lds == 0 and not [o for o in ops if o.startswith(("global_atomic", "ds_"))], (name, sorted(set(ops)))
        else:
            assert lds == 0 and "global_store_dwordx4" in ops and not [o for o in ops if o.startswith("global_atomic")], (name, sorted(set(ops)))
