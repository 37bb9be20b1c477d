"""The block index (acm_index_file), the host window stager (acm_stage_window) and the window semantics of
acm_batch_decode_windows, on the CPU (libacm_amd/csrc/acm_stage.cpp, acm_batch_windows.cpp; include/acm_hip.h).

The yardstick throughout is acm_stage_file over the whole file: the index must report what it reports, and a window staged through
the index must be exactly the slice of what it writes - indices, headers and H1 patches (sample positions and values)."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN_DIR, golden_file, make_stream
from libacm_amd import _build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACM_ERR_NOT_ACM, ACM_ERR_CORRUPT = -3, -6

INFO_FIELDS = [f for f, _ in capi.StageInfo._fields_]


def info_tuple(info):
    return tuple(int(getattr(info, f)) for f in INFO_FIELDS)


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, "acm", "*.acm")))


def synthetic_streams():
    k = 0
    for level in (0, 4, 5, 7, 9, 12, 15):
        for rows in (1, 2, 3, 16, 255):
            for ch in (1, 2):
                k += 1
                yield (level, rows, ch), make_stream(7000 + k, level, rows, 5 if (rows << level) < (1 << 18) else 3, channels=ch, cut=k % 5,
                                                     mix=k % 2)


def h1_streams():
    """the stale-table streams of test_host_parser / test_gpu_parity: indices outside the block's table, resolved against earlier blocks"""
    out = [make_stream(800 + seed, 5, 7, 8, mix=1, allow_out_of_range=1, prime_table=1, pwr_min=0, pwr_max=15, val_min=0, val_max=65535)
           for seed in range(12)]
    out += [make_stream(900 + lv, lv, rows, 8, mix=1, allow_out_of_range=1, prime_table=1, pwr_min=0, pwr_max=6)
            for lv, rows in ((3, 4), (5, 16), (7, 16), (9, 4))]
    return out


def check_index(data, force_chans=0):
    rc, _ = capi.probe(data, force_chans)
    if rc != 0:
        with pytest.raises(ValueError):
            capi.index_file(data, force_chans)
        return None, None
    st = capi.stage_file(data, force_chans)
    marks, info = capi.index_file(data, force_chans)
    assert info_tuple(info) == info_tuple(st.info)
    assert marks.size == st.info.blocks + 1
    assert np.array_equal(marks["val"][:-1], st.hdr[:, 0]) and np.array_equal(marks["pwr"][:-1], st.hdr[:, 1])
    assert marks["val"][-1] == 0 and marks["pwr"][-1] == 0
    assert np.all(np.diff(marks["bit"].astype(np.int64)) > 0)
    assert marks["bit"][0] == 8 * info.header_bytes if st.info.blocks else True
    assert marks["bit"][-1] <= 8 * (len(data) + 1)
    return st, marks


def test_index_matches_stage_file():
    n = 0
    for path in golden_files():
        with open(path, "rb") as f:
            data = f.read()
        for fc in (0, -1, 2):
            st, _ = check_index(data, fc)
            n += st is not None
    assert n > 300
    for key, data in synthetic_streams():
        st, marks = check_index(data)
        assert st.info.blocks >= 3 and st.info.end_status == 0, key
    st, _ = check_index(golden_file("f5_wavc"))
    assert st.info.wavc == 1 and st.info.header_bytes == 42 and st.info.blocks > 0
    for data in h1_streams():
        st, _ = check_index(data)
        assert st.info.blocks == 8


def test_index_of_truncated_files():
    rng = np.random.default_rng(20240)
    bases = [make_stream(7400, 5, 16, 6, mix=1), make_stream(7401, 0, 3, 40), make_stream(7402, 9, 4, 5, channels=2),
             golden_file("f5_wavc"), make_stream(7403, 2, 1, 50, mix=1)]
    ends = set()
    for data in bases:
        assert len(data) > 100
        cuts = sorted({int(c) for c in rng.choice(len(data) + 1, size=64, replace=False)} | {len(data) - 1, len(data) - 2, len(data) - 3, 14, 15})
        assert len(cuts) >= 64
        for c in cuts:
            st, marks = check_index(data[:c])
            if st is not None:
                ends.add(st.info.end_status)
                if st.info.blocks:
                    check_windows(data[:c], st, marks, [(st.info.blocks - 1, 1), (0, st.info.blocks + 1), (st.info.blocks, 1)])
    assert len(ends) >= 2                       # clean ends and errors both occurred


def patch_slice(st, first, nblocks):
    bl = st.block_len
    if st.patches is None:
        return []
    return [(p.sample - first * bl, p.value) for p in st.patches if first * bl <= p.sample < (first + nblocks) * bl]


def check_windows(data, st, marks, ranges, force_chans=0):
    bl = st.block_len
    nb = st.info.blocks
    for first, count in ranges:
        rc, w = capi.stage_window(data, marks, first, count, force_chans)
        assert rc == 0, (first, count, rc)
        want = max(0, min(count, nb - first))
        assert w.info.blocks == want, (first, count)
        assert w.info.end_status == (st.info.end_status if first + count > nb else 0), (first, count)
        assert np.array_equal(w.idx, st.idx[first * bl:(first + want) * bl]), (first, count)
        assert np.array_equal(w.hdr, st.hdr[first:first + want]), (first, count)
        got = [(p.sample, p.value) for p in w.patches] if w.patches is not None else []
        assert got == patch_slice(st, first, want), (first, count)
        assert w.info.npatches == len(got)
        assert (w.info.level, w.info.rows, w.info.cols, w.info.channels, w.info.total_values) == \
               (st.info.level, st.info.rows, st.info.cols, st.info.channels, st.info.total_values)


def window_ranges(nb):
    return [(0, 1), (0, 2), (nb // 2, 2), (nb // 2, 1), (nb - 1, 1), (nb - 2, 5), (1, 0), (0, nb), (nb, 3), (1, nb - 1)]


def test_stage_window_is_a_slice_of_stage_file():
    for key, data in synthetic_streams():
        st = capi.stage_file(data)
        marks, _ = capi.index_file(data)
        check_windows(data, st, marks, window_ranges(st.info.blocks))
    for name in ("f5_wavc", "f7_src", "f4_base", "f7_corrupt_block2"):
        data = golden_file(name)
        st = capi.stage_file(data)
        marks, _ = capi.index_file(data)
        if st.info.blocks >= 2:
            check_windows(data, st, marks, window_ranges(st.info.blocks))
    data = make_stream(7500, 6, 8, 9, channels=1)
    st = capi.stage_file(data, 2)
    marks, _ = capi.index_file(data, 2)
    check_windows(data, st, marks, window_ranges(st.info.blocks), force_chans=2)


def test_stage_window_resolves_stale_table_reads_from_the_marks():
    """H1: a window entered behind the blocks that left the stale entries must patch with the values those blocks left - the table
    history is seeded from the marks' (val, pwr)"""
    deep = 0
    for data in h1_streams():
        st = capi.stage_file(data)
        marks, _ = capi.index_file(data)
        nb = st.info.blocks
        assert st.info.npatches > 0
        check_windows(data, st, marks, window_ranges(nb) + [(b, 1) for b in range(nb)] + [(b, nb) for b in range(nb)])
        deep += len(patch_slice(st, nb // 2, nb - nb // 2))
    assert deep > 0                             # patches did occur in windows that start in mid-stream


def test_bad_indices_are_refused_or_end_with_a_status():
    a = make_stream(7600, 5, 16, 8, mix=1)
    b = make_stream(7601, 5, 16, 8, mix=1)      # the same geometry, other contents
    st = capi.stage_file(a)
    marks, _ = capi.index_file(a)
    foreign, _ = capi.index_file(b)
    bl = st.block_len

    def harmless(rc, w, first):
        """refused, ended with a status, or the true slice"""
        if rc != 0:
            assert rc == capi.ERR_ARG
            return "refused"
        if w.info.end_status != 0:
            return "status"
        assert np.array_equal(w.idx, st.idx[first * bl:(first + w.info.blocks) * bl])
        assert np.array_equal(w.hdr, st.hdr[first:first + w.info.blocks])
        return "exact"

    m = marks.copy()
    m["bit"][3], m["bit"][4] = marks["bit"][4], marks["bit"][3]
    assert capi.stage_window(a, m, 0, 8)[0] == capi.ERR_ARG                     # not monotone
    m = marks.copy()
    m["bit"][5] = 8 * len(a) + 1000
    assert capi.stage_window(a, m, 0, 8)[0] == capi.ERR_ARG                     # beyond the file
    m = marks.copy()
    m["bit"][8] = 8 * len(a) + 1000
    assert capi.stage_window(a, m, 0, 2)[0] == capi.ERR_ARG                     # ... in the end entry
    m = marks.copy()
    m["bit"][0] = 8
    assert capi.stage_window(a, m, 0, 2)[0] == capi.ERR_ARG                     # inside the header
    assert capi.stage_window(a, marks, 9, 1)[0] == capi.ERR_ARG                 # block_first beyond the index
    assert capi.stage_window(a, marks, 3, 1, nblocks_indexed=2)[0] == capi.ERR_ARG
    outcomes = set()
    for first in range(8):
        rc, w = capi.stage_window(a, foreign, first, 8 - first)
        outcomes.add(harmless(rc, w, first))
        if rc == 0 and first > 0:
            assert w.info.end_status != 0 and w.info.blocks == 0                # a foreign mark does not start a block of this file
    assert "status" in outcomes or "refused" in outcomes
    for shift in (1, 3, 8, -1):
        m = marks.copy()
        m["bit"][4] = int(m["bit"][4]) + shift
        for first, count in ((4, 1), (3, 2), (0, 8)):
            rc, w = capi.stage_window(a, m, first, count)
            assert harmless(rc, w, first) != "exact" or w.info.blocks < count
    m = marks.copy()
    m["val"][2] ^= 0x10
    rc, w = capi.stage_window(a, m, 2, 1)
    assert rc == 0 and w.info.end_status == ACM_ERR_CORRUPT and w.info.blocks == 0
    m = marks.copy()
    m["pwr"][2] = 16
    assert capi.stage_window(a, m, 0, 1)[0] == capi.ERR_ARG
    rc, w = capi.stage_window(b"RIFF" + bytes(60), marks, 0, 1)
    assert rc == ACM_ERR_NOT_ACM


def test_index_and_stager_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "fuzz_index")
    csrc = os.path.join(ROOT, "libacm_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "fuzz_index.cpp")] + \
          [os.path.join(csrc, f) for f in ("acm_stage.cpp", "acm_fill.cpp", "acm_pack.cpp", "acm_kernel_geo.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, "-o", exe] + src + ["-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and "sanitize" in r.stdout and "cannot find" in r.stdout:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stdout
    files = sorted(glob.glob(os.path.join(GOLDEN_DIR, "acm", "f[12357]_*.acm")))[::3]
    extra = [make_stream(7700, 5, 16, 8, mix=1), make_stream(7701, 5, 16, 8, mix=1), make_stream(7702, 0, 3, 30), make_stream(7703, 11, 16, 3)] + \
        h1_streams()[:4] + h1_streams()[12:]
    for k, data in enumerate(extra):
        path = str(tmp_path / ("s%02d.acm" % k))
        with open(path, "wb") as f:
            f.write(data)
        files.append(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "24"] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "index fuzz ok" in r.stdout, r.stdout[-3000:]


# --------------------------------------------------------------------------- window semantics, in pure Python
def expected_window(st, status, first_word, max_words):
    """(words, status, b0, nblocks) of a window over a stream whose acm_stage_file result is `st` (None: not ACM; status then says why):
    the rule of include/acm_hip.h.  tests/test_gpu_windows.py takes its expected values from here."""
    whole = st.words if st is not None else 0
    words = 0 if first_word >= whole else min(max_words, whole - first_word)
    end = st.info.end_status if st is not None else status
    out_status = 0 if words == max_words else end
    if not words:
        return 0, out_status, 0, 0
    cols, rows = st.info.cols, st.info.rows
    first_row, last_row = first_word // cols, (first_word + words - 1) // cols
    b0 = max(first_row - 2, 0) // rows
    return words, out_status, b0, last_row // rows + 1 - b0


def test_window_semantics_table():
    data = make_stream(7800, 5, 4, 6, cut=7)            # 32 columns, 4 rows: 128 samples a block, 761 in all
    st = capi.stage_file(data)
    assert st.words == 761 and st.info.blocks == 6
    table = [
        # first, max      words status b0 blocks
        ((0, 10),         (10, 0, 0, 1)),
        ((0, 128),        (128, 0, 0, 1)),
        ((0, 129),        (129, 0, 0, 2)),
        ((5, 3),          (3, 0, 0, 1)),
        ((128, 1),        (1, 0, 0, 2)),                # row 4: the halo rows 2, 3 are in block 0
        ((191, 1),        (1, 0, 0, 2)),                # row 5: halo rows 3, 4
        ((192, 1),        (1, 0, 1, 1)),                # row 6: halo rows 4, 5 - block 1 alone
        ((300, 200),      (200, 0, 1, 3)),
        ((0, 761),        (761, 0, 0, 6)),
        ((0, 10000),      (761, 0, 0, 6)),              # a stream that simply ended: its own end status, ACM_OK
        ((760, 5),        (1, 0, 5, 1)),
        ((761, 5),        (0, 0, 0, 0)),
        ((5000, 5),       (0, 0, 0, 0)),
        ((10, 0),         (0, 0, 0, 0)),
    ]
    for (first, count), want in table:
        assert expected_window(st, 0, first, count) == want, (first, count)
    cut = capi.stage_file(data[:len(data) // 2])
    assert cut.info.end_status < 0 and 0 < cut.words < 761
    assert expected_window(cut, 0, 0, cut.words) == (cut.words, 0, 0, cut.info.blocks)
    assert expected_window(cut, 0, 0, cut.words + 1)[:2] == (cut.words, cut.info.end_status)
    assert expected_window(cut, 0, cut.words, 1)[:2] == (0, cut.info.end_status)
    assert expected_window(None, ACM_ERR_NOT_ACM, 0, 1) == (0, ACM_ERR_NOT_ACM, 0, 0)
    assert expected_window(None, ACM_ERR_NOT_ACM, 0, 0) == (0, 0, 0, 0)


def test_window_pcm_words_bound():
    data = make_stream(7800, 5, 4, 6, cut=7)
    files = [data, b"not an acm file at all", data[:len(data) // 2]]
    wins = [(0, 0, 10), (0, 5, 3), (0, 300, 200), (0, 760, 5), (0, 761, 5), (1, 0, 100), (2, 0, 10000), (0, 31, 64), (7, 0, 5)]
    st = [capi.stage_file(files[0]), None, capi.stage_file(files[2])]
    need = 0
    for f, first, count in wins:
        if f < 3 and st[f] is not None:
            words = expected_window(st[f], 0, first, count)[0]
            need += (first % 32 + words + 63) // 64 * 64 if words else 0
    got = capi.batch_window_pcm_words(files, wins)
    assert need <= got <= need + 64 * len(wins) + 10000     # an upper bound from the headers alone: never less than the call will use


def test_no_device_is_an_error_not_a_fallback():
    data = make_stream(7800, 5, 4, 6)
    marks, info = capi.index_file(data)
    bufs, items, ix, wins, keep = capi._window_tables([data], [marks], [(0, 0, 100)])
    assert ix[0].blocks == 6 and ix[0].end_status == 0
    tm = capi.WindowTiming()
    assert capi.lib().acm_batch_decode_windows(None, items, 1, ix, wins, 1, None, C.byref(tm)) == capi.ERR_NO_DEVICE
    assert C.sizeof(capi.BlockMark) == 16 and capi.BLOCK_MARK_DT.itemsize == 16
    assert C.sizeof(capi.BatchIndex) == 16 and C.sizeof(capi.BatchWindow) == 80 and C.sizeof(capi.WindowTiming) == 88


def test_build_index():
    from libacm_amd import batch
    files = [make_stream(7900 + k, 5, 8, 4 + k) for k in range(5)] + [b"garbage"]
    ix = batch.build_index(files, threads=3)
    assert [a.size for a in ix] == [5, 6, 7, 8, 9, 0]
    for f, a in zip(files[:5], ix):
        assert np.array_equal(a, capi.index_file(f)[0])


# --------------------------------------------------------------------------- build and generated-code invariants
def test_block_walk_kernel_owns_m0_and_has_no_scratch(tmp_path):
    """acm_parse_scan_blocks uses the v_writelane-through-m0 idiom of acm_parse_scan_wave: what tests/test_isa_invariants.py demands of
    that kernel holds for this one - it cross-compiles for gfx950, nothing the compiler generated in it touches m0, no scratch"""
    out = tmp_path / "acm_parse.s"
    cmd = [_build.HIPCC, "-O3", "-std=c++17", "--offload-arch=" + _build.GFX, "-I", _build.INC, "-I", _build.CSRC,
           "--cuda-device-only", "-S", "-o", str(out), os.path.join(_build.CSRC, "acm_parse.hip")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    asm = out.read_text()
    m = re.search(r"^(_ZN\S*acm_parse_scan_blocks\S*):", asm, re.M)
    assert m
    body = asm[m.end():asm.index(".Lfunc_end", m.end())].split("\n")
    by_hand, mine, writes, atomics = False, 0, 0, 0
    for l in body:
        t = l.strip()
        if t.startswith(";;#ASMSTART"):
            by_hand = True
        elif t.startswith(";;#ASMEND"):
            by_hand = False
        elif t and not t.startswith(";"):
            code = t.split(";")[0]
            if by_hand:
                mine += "m0" in code
                writes += code.startswith("v_writelane_b32")
            else:
                assert not re.search(r"\bm0\b", code), t
                assert not t.startswith("scratch_"), t
                atomics += code.startswith(("global_atomic_", "flat_atomic_"))
                assert not re.match(r"s_(buffer_)?atomic|s_(buffer_|scratch_)?store|s_dcache_(wb|discard)", code), t
    assert writes >= 1 and mine == 2 * writes
    assert atomics >= 2                         # the job's record is raised by vector atomics
    md = re.search(r"\.amdhsa_kernel \S*acm_parse_scan_blocks\S*\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size (\d+)", asm)
    assert md and md.group(1) == "0"


def test_no_scalar_memory_writes_in_any_source():
    """scalar stores, scalar atomics and scalar cache write-backs are not used anywhere: values go out through vector stores"""
    words = re.compile("|".join(["s_" + "store_dword", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic_", "s_buffer_" + "atomic",
                                 "s_dcache_" + "wb", "s_dcache_" + "discard"]), re.I)
    n = 0
    tops = [os.path.join(ROOT, d) for d in ("include", "libacm_amd", "tests", "oracle", "profiles", "examples")]
    walks = [w for top in tops for w in os.walk(top)] + [(ROOT, [], [f for f in os.listdir(ROOT) if os.path.isfile(os.path.join(ROOT, f))])]
    for base, dirs, names in walks:
        if any(part in ("_ref", "_build", "__pycache__", "lib", "bin") for part in os.path.relpath(base, ROOT).split(os.sep)):
            continue
        for name in names:
            if name.endswith((".hip", ".cpp", ".c", ".h", ".hpp", ".inc", ".py", ".sh", ".s", ".S", ".asm")):
                with open(os.path.join(base, name), errors="replace") as f:
                    assert not words.search(f.read()), os.path.join(base, name)
                n += 1
    assert n > 50
