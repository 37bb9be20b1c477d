"""Dense crop batches without a GPU: the device-free half of acm_batch_decode_windows_dense (libacm_amd/csrc/acm_dense_layout.cpp), the
case list of tests/dense_crops.py, and the code the compiler makes of the gather kernel (libacm_amd/csrc/acm_dense.hip).

  * acmk_dense_layout_visit() against a pure-Python model: which windows are turned away for their channel count and reach the window
    layout asking for nothing, what every window is told, the output size, the row table - { where the window's first sample sits in the
    intermediate arena, samples to copy } - and where the table travels; every call the dense writer refuses as a whole; a window of
    which staging left nothing.  The layout underneath is the model of tests/test_window_layout.py.
  * what the case list reaches, asserted here so that the GPU tests over the same list cannot pass vacuously.
  * acm_dense.hip compiled to gfx950 assembly: no scratch, 16-byte global loads and stores in every build of the kernel."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_crops as DC
import test_window_layout as WL
from libacm_amd import _build, capi

TOTALS = ("frames", "row_words", "channels", "planar", "f32", "out_words", "pcm_arena_words", "blocks_parsed", "table_off", "table_bytes", "rc")
PCM_SLACK = 64                  # ACM_DENSE_PCM_SLACK
FAKE_PTR = 0x1000


def _lib():
    L = capi.lib()
    L.acmk_dense_layout_visit.argtypes = [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, WL.VISIT, C.c_void_p]
    return L


def call(items, wins, frames, channels, dense_flags=0, parse=capi.PARSE_HOST, f32=False, d_pcm=FAKE_PTR, d_pcm_words=None, fmt=capi.FMT_S16LE,
         batch_flags=0, prestaged=None, final_words=None, no_dense=False):
    """acmk_dense_layout_visit -> (rc, {table: uint64 array})"""
    n, nwin = len(items), len(wins)
    info = (capi.StageInfo * max(n, 1))()
    length, whole = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
    ok, end_status, blocks = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint32)
    marks = (C.c_void_p * max(n, 1))()
    for i, it in enumerate(items):
        f = it.info
        info[i] = capi.StageInfo(f.level, f.rows, f.cols, f.channels, f.channels, 22050, f.total_values, 0, f.blocks, f.end_status, 0, f.header_bytes)
        length[i], whole[i], ok[i], end_status[i], blocks[i] = it.len, it.whole, it.ok, it.end_status, f.blocks
        marks[i] = it.marks.ctypes.data if it.marks is not None else None
    win3 = np.array(wins, dtype=np.uint64).reshape(-1)
    if d_pcm_words is None:
        d_pcm_words = nwin * frames * channels
    opts = capi.BatchOpts(0, fmt, 4, 0, parse, batch_flags | (capi.BATCH_PCM_F32 if f32 else 0), d_pcm, d_pcm_words, prestaged)
    dense = capi.DenseOpts(frames, channels, dense_flags)
    final = None if final_words is None else np.array(final_words, dtype=np.uint64)
    tables = {}

    def visit(_ctx, name, data, elem_bytes, count):
        assert name.decode() not in tables and elem_bytes % 8 == 0
        tables[name.decode()] = np.frombuffer(C.string_at(data, elem_bytes * count), dtype="<u8").reshape(count, elem_bytes // 8).copy()
    rc = _lib().acmk_dense_layout_visit(info, length.ctypes.data, ok.ctypes.data, end_status.ctypes.data, whole.ctypes.data, marks, blocks.ctypes.data,
                                        n, win3.ctypes.data if nwin else None, nwin, C.byref(opts), None if no_dense else C.byref(dense),
                                        final.ctypes.data if final is not None else None, WL.VISIT(visit), None)
    tot = dict(zip(TOTALS, tables["totals"].reshape(-1).astype(np.int64).tolist()))
    assert tot["rc"] == rc
    return rc, tables, tot


def model(items, wins, frames, channels, planar, parse, f32, final_words=None):
    """the tables of an accepted call, as acm_dense_layout.h words them"""
    R = frames * channels
    rejected = [int(f < len(items) and bool(items[f].ok) and items[f].info.channels != channels) for f, first, count in wins]
    inner = [(f, first, 0 if rej else count) for (f, first, count), rej in zip(wins, rejected)]
    lay = WL.model(WL.Case("", items, inner, parse=parse))
    assert lay["totals"]["rc"] == 0
    report, rows = [], []
    for k, s in enumerate(lay["slots"]):
        report.append((capi.ERR_ARG if rejected[k] else s["status"], s["words"], k * R, k * R, R))
        count = min(s["words"], s["words"] if final_words is None else final_words[k]) if s["active"] else 0
        rows.append((s["dev_off"], count) if count else (0, 0))
    t = lay["totals"]
    tot = dict(frames=frames, row_words=R, channels=channels, planar=int(planar), f32=int(f32), out_words=len(wins) * R,
               pcm_arena_words=t["pcm_total"] + PCM_SLACK, blocks_parsed=t["blocks_parsed"],
               table_off=WL.round_up(t["jobs_bytes"] + t["bjobs_bytes"] + t["res_bytes"], 64), table_bytes=16 * len(wins), rc=0)
    return {"wins": inner, "rejected": rejected, "report": report, "rows": rows, "totals": tot}


@pytest.fixture(scope="module")
def items():
    return [DC.layout_item(f) for f in DC.files()]


def signed(a):
    return [tuple(int(v) for v in r) for r in a.astype(np.int64)]


# ---------------------------------------------------------------------------------------------------------------- the row table

@pytest.mark.parametrize("parse", [capi.PARSE_HOST, capi.PARSE_DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
def test_row_table_equals_the_model(items, parse, planar):
    for case in DC.cases():
        for f32 in (False, True):
            rc, got, tot = call(items, case.windows, case.frames, case.channels, dense_flags=int(planar), parse=parse, f32=f32)
            want = model(items, case.windows, case.frames, case.channels, planar, parse, f32)
            assert rc == 0 and tot == want["totals"], (case.name, tot, want["totals"])
            assert signed(got["wins"]) == want["wins"] and got["rejected"].reshape(-1).tolist() == want["rejected"], case.name
            assert signed(got["report"]) == want["report"] and signed(got["rows"]) == want["rows"], case.name
            # ... and what the case builder expects of the call, window by window: the two descriptions of the contract agree
            nblocks = 0
            for k in range(len(case.windows)):
                words, status, nb = case.expect(k)
                nblocks += nb
                assert want["report"][k][:2] == (status, words) and words == case.delivers(k), (case.name, k, case.windows[k])
                assert want["rejected"][k] == int(case.rejected(k))
            assert tot["blocks_parsed"] == nblocks


def test_rows_lie_inside_their_slots(items):
    """every record names samples the window layout gave the window: inside the arena the call asks for, never across a slot's end, and
    the 16-byte lines that hold a record's samples stay inside the slot (slots are runs of 64 samples)"""
    for case in DC.cases():
        rc, got, tot = call(items, case.windows, case.frames, case.channels, parse=capi.PARSE_DEVICE)
        for src, count in signed(got["rows"]):
            if count:
                lo, hi = src * 2 // 16 * 16, -(-(src + count) * 2 // 16) * 16
                assert lo // 128 * 128 <= lo and hi <= -(-(src + count) // 64) * 128 <= 2 * (tot["pcm_arena_words"] - PCM_SLACK), (case.name, src, count)
            else:
                assert src == 0


def test_a_window_staging_left_nothing_of(items):
    """the host stager turns windows away during the call (a stale index): their records copy nothing, the others are unchanged"""
    case = DC.cases()[0]
    rc, before, _ = call(items, case.windows, case.frames, case.channels)
    final = [int(r[1]) for r in before["report"]]
    hit = [k for k, w in enumerate(final) if w][1:8:3]
    assert len(hit) == 3
    for k in hit:
        final[k] = 0
    rc, got, tot = call(items, case.windows, case.frames, case.channels, final_words=final)
    want = model(items, case.windows, case.frames, case.channels, False, capi.PARSE_HOST, False, final_words=final)
    assert rc == 0 and signed(got["rows"]) == want["rows"]
    for k, (a, b) in enumerate(zip(signed(before["rows"]), signed(got["rows"]))):
        assert b == ((0, 0) if k in hit else a), k
    assert signed(got["report"]) == signed(before["report"])            # (what the window is told then is the stager's, in the driver)


def test_every_refusal(items):
    """ACMHIP_ERR_ARG for the call as a whole, and no table but the totals"""
    wins, T = [(0, 8, 32), (2, 16, 64)], 64
    ok = dict(frames=T, channels=1)
    rc, tables, tot = call(items, wins, **ok)
    assert rc == 0 and tot["out_words"] == 2 * T
    refusals = {
        "no acm_dense_opts": dict(ok, no_dense=True),
        "frames == 0": dict(ok, frames=0, d_pcm_words=1000),
        "channels == 0": dict(ok, channels=0, d_pcm_words=1000),
        "channels == 3": dict(ok, channels=3, d_pcm_words=1000),
        "unknown dense flag": dict(ok, dense_flags=2),
        "unknown dense flag beside a known one": dict(ok, dense_flags=0x80000001),
        "no output": dict(ok, d_pcm=None),
        "output one sample short": dict(ok, d_pcm_words=2 * T - 1),
        "big-endian": dict(ok, fmt=capi.FMT_S16BE),
        "unsigned": dict(ok, fmt=capi.FMT_U16LE),
        "prestaged": dict(ok, prestaged=FAKE_PTR),
        "packed staging": dict(ok, batch_flags=capi.BATCH_STAGE_PACKED),
        "rows past 64 bits": dict(ok, frames=1 << 63, d_pcm_words=(1 << 64) - 1),
    }
    for what, kw in refusals.items():
        rc, tables, tot = call(items, wins, **kw)
        assert rc == capi.ERR_ARG and list(tables) == ["totals"], what
    for what, bad, ch in (("max_words > R", (0, 0, T + 1), 1), ("max_words > R, stereo", (1, 0, 2 * T + 2), 2), ("odd first_word", (1, 3, 8), 2),
                          ("odd max_words", (1, 4, 7), 2), ("odd first_word of a window that asks for nothing", (3, 1, 0), 2)):
        rc, tables, tot = call(items, wins[:1] + [bad] + wins[1:], frames=T, channels=ch)
        assert rc == capi.ERR_ARG and list(tables) == ["totals"], what
    # on the edge, accepted: exactly R samples, exactly enough room, float output, no windows at all
    assert call(items, [(0, 0, T), (1, 3, T)], frames=T, channels=1)[0] == 0
    assert call(items, [(1, 2, 2 * T)], frames=T, channels=2, f32=True, dense_flags=1)[0] == 0
    rc, tables, tot = call(items, [], frames=T, channels=2)
    assert rc == 0 and list(tables) == ["totals"] and tot["out_words"] == 0 and tot["table_bytes"] == 0


# ---------------------------------------------------------------------------------------------------------------- the case list

def test_case_list_reaches_what_the_kernel_can_get_wrong():
    cases = DC.cases()
    assert sorted((c.channels, c.frames) for c in cases) == [(1, 37), (1, 64), (2, 37), (2, 64)]
    assert {c.row % 8 == 0 for c in cases if c.channels == 1} == {c.row % 8 == 0 for c in cases if c.channels == 2} == {True, False}
    residues, lengths, kinds = set(), {c.name: set() for c in cases}, set()
    levels = set()
    for c in cases:
        n_deliver = 0
        for k, (f, first, count) in enumerate(c.windows):
            words = c.delivers(k)
            n_deliver += words > 0
            lengths[c.name].add(words)
            if f >= len(DC.files()):
                kinds.add("no such file")
                continue
            src = DC.files()[f]
            if c.rejected(k):
                kinds.add("another channel count")
            elif not src.acm:
                kinds.add("not ACM")
            elif first >= src.words:
                kinds.add("behind the end")
            elif words < count:
                kinds.add("clipped by the end" if src.end_status == 0 else "clipped by a stream that breaks off")
            if words >= 9:
                residues.add(first % 8)
                levels.add((src.info.level, src.channels))
            if words and first // src.st.block_len != (first + words - 1) // src.st.block_len:
                kinds.add("across a block boundary")
        assert 4 * n_deliver >= 3 * len(c.windows), (c.name, n_deliver, len(c.windows))
        assert {0, c.channels, 8, c.row - c.channels, c.row} <= lengths[c.name], (c.name, sorted(lengths[c.name]))
    assert residues == set(range(8)), sorted(residues)
    assert all({7, 9} <= lengths[c.name] for c in cases if c.channels == 1)
    assert kinds == {"no such file", "another channel count", "not ACM", "behind the end", "clipped by the end", "clipped by a stream that breaks off",
                     "across a block boundary"}, sorted(kinds)
    assert levels == {(1, 1), (1, 2), (5, 1), (5, 2), (9, 1), (9, 2)}, sorted(levels)


def test_expected_rows_follow_the_formula():
    """the builder's vectorised rows against the contract's formula spelled out element by element, on a sample of each case"""
    rng = np.random.default_rng(0xD0)
    for c in DC.cases():
        inter, planar = c.rows(False), c.rows(True)
        assert inter.shape == planar.shape == (len(c.windows), c.row) and inter.any()
        for k in rng.choice(len(c.windows), 12, replace=False):
            f, first, count = c.windows[k]
            words = c.delivers(k)
            whole = DC.files()[f].pcm if f < len(DC.files()) else None
            for e in range(c.row):
                assert inter[k, e] == (whole[first + e] if e < words else 0)
                j = (e % c.frames) * c.channels + e // c.frames
                assert planar[k, e] == (whole[first + j] if j < words else 0)


# ---------------------------------------------------------------------------------------------------------------- the kernel's code

@pytest.fixture(scope="module")
def kernel_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "acm_dense.s"
    cmd = [_build.HIPCC, "-O3", "-std=c++17", "--offload-arch=" + _build.GFX, "-I", _build.INC, "-I", _build.CSRC,
           "--cuda-device-only", "-S", "-o", str(out), os.path.join(_build.CSRC, "acm_dense.hip")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return out.read_text()


def test_kernel_has_wide_accesses_and_no_scratch(kernel_asm):
    """all eight builds ({int16, float32} x {interleaved, planes} x {temporal, non-temporal stores}): a body of global_load_dwordx4 and
    global_store_dwordx4 - stereo planes read up to three lines a vector, float32 stores two - no flat or scratch access, no private
    segment, no LDS"""
    bodies = {}
    for m in re.finditer(r"^(_ZN\S*acm_dense_rows\S*):", kernel_asm, re.M):
        bodies[m.group(1)] = kernel_asm[m.end():kernel_asm.index(".Lfunc_end", m.end())]
    assert len(bodies) == 8, sorted(bodies)
    for name, body in bodies.items():
        ops = re.findall(r"^\s+((?:global|flat|scratch|buffer|ds)_\w+)", body, re.M)
        stride2, f32 = "Li2E" in name, "rowsIf" in name
        assert ops.count("global_load_dwordx4") == (3 if stride2 else 2), (name, ops)
        assert ops.count("global_store_dwordx4") == (2 if f32 else 1), (name, ops)
        assert not [o for o in ops if o.startswith(("flat_", "scratch_", "buffer_", "ds_"))], (name, ops)
        # narrow accesses are the head, the tail and the vector a short row ends in: 16-bit loads; 2- or 4-byte stores
        assert set(ops) <= {"global_load_dwordx4", "global_store_dwordx4", "global_load_sshort", "global_load_ushort", "global_load_short_d16",
                            "global_load_short_d16_hi", "global_store_short", "global_store_dword"}, (name, sorted(set(ops)))
        meta = re.search(r"\.name:\s+%s\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)" % re.escape(name), kernel_asm)
        assert meta and int(meta.group(1)) == 0, name
        desc = kernel_asm[kernel_asm.index(".amdhsa_kernel " + name):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc) and re.search(r"\.amdhsa_group_segment_fixed_size 0\b", desc), name
