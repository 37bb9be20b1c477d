"""Dense crop batches over mono and stereo files without a GPU: ACM_DENSE_MIX in the device-free half of acm_batch_decode_windows_dense
(libacm_amd/csrc/acm_dense_layout.cpp), the case list of tests/dense_mix.py, and the code the compiler makes of the converting gather
kernel (libacm_amd/csrc/acm_dense_mix.hip).

  * acmk_dense_layout_visit() with the flag against a pure-Python model (tests/dense_mix.py::model): no window is turned away for its
    channel count, every row has a mode, a converting row carries it above its count of SOURCE samples, the "mix" table says whether the
    converting kernel is needed, and blocks_parsed counts the converted windows' blocks.
  * the refusals in the source's own units, and what lies on their edge.
  * calls without the flag: the tables of tests/test_dense_crops.py's model and no other; the flag over one channel count: the same
    rows and the verdict "existing kernel".
  * what the case list reaches, asserted here so that the GPU tests over the same list cannot pass vacuously.
  * acm_dense_mix.hip compiled to gfx950 assembly: 16-byte global loads and stores in every build, no scratch, no LDS."""
import os
import re
import subprocess

import numpy as np
import pytest

import dense_crops as DC
import dense_mix as DM
import test_dense_crops as TD
from libacm_amd import _build, capi

MIX = capi.DENSE_MIX
PLAIN_TABLES = ["wins", "rejected", "report", "rows", "totals"]


@pytest.fixture(scope="module")
def items():
    return [DC.layout_item(f) for f in DC.files()]


def flat(table):
    return table.reshape(-1).astype(np.int64).tolist()


# ---------------------------------------------------------------------------------------------------------------- the layout

@pytest.mark.parametrize("parse", [capi.PARSE_HOST, capi.PARSE_DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
def test_layout_equals_the_model(items, parse, planar):
    for case in DM.cases():
        for f32 in (False, True):
            rc, got, tot = TD.call(items, case.windows, case.frames, case.channels, dense_flags=MIX | int(planar), parse=parse, f32=f32)
            want = DM.model(items, case.windows, case.frames, case.channels, planar, parse, f32)
            assert rc == 0 and tot == want["totals"], (case.name, tot, want["totals"])
            assert list(got) == PLAIN_TABLES[:-1] + ["mix", "totals"]
            assert TD.signed(got["wins"]) == want["wins"] and flat(got["rejected"]) == want["rejected"], case.name
            assert TD.signed(got["report"]) == want["report"] and TD.signed(got["rows"]) == want["rows"], case.name
            assert flat(got["mix"]) == want["mix"] and want["mix"][-1] == 1, case.name
            # ... and what the case builder expects of the call, window by window: the two descriptions of the contract agree
            nblocks = 0
            for k in range(len(case.windows)):
                words, status, nb = case.expect(k)
                nblocks += nb
                assert want["report"][k][:2] == (status, words) and words == case.delivers(k), (case.name, k, case.windows[k])
                assert want["mix"][k] == case.mode(k, planar)
            assert tot["blocks_parsed"] == nblocks


def test_rows_lie_inside_their_slots(items):
    """a converting row's record names SOURCE samples: they lie inside the slot the window layout gave the window, and so do the
    aligned 16-byte lines that hold them - all the kernel loads - since a slot is a run of 64 samples from a multiple of 64 on"""
    for case in DM.cases():
        rc, got, tot = TD.call(items, case.windows, case.frames, case.channels, dense_flags=MIX, parse=capi.PARSE_DEVICE)
        slots = TD.WL.model(TD.WL.Case("", items, case.windows, parse=capi.PARSE_DEVICE))["slots"]
        for k, (src, word) in enumerate(TD.signed(got["rows"])):
            count, mode = word & ((1 << DM.MODE_SHIFT) - 1), word >> DM.MODE_SHIFT
            assert count == case.delivers(k) and mode == (case.mode(k, False) if count and case.mode(k, False) >= DM.DOWN else 0)
            if count:
                s = slots[k]
                assert s["slot_off"] % 64 == 0 and s["slot_words"] % 64 == 0 and s["slot_off"] + s["slot_words"] <= tot["pcm_arena_words"] - TD.PCM_SLACK
                assert s["slot_off"] <= src and src + count <= s["slot_off"] + s["slot_words"], (case.name, k)
                lo, hi = src * 2 // 16 * 16, -(-(src + count) * 2 // 16) * 16          # bytes of the lines that hold a sample
                assert 2 * s["slot_off"] <= lo and hi <= 2 * (s["slot_off"] + s["slot_words"]), (case.name, k)
                assert mode != DM.DOWN or src % 2 == 0          # a stereo window starts on a dword of the arena


def test_converting_windows_staging_left_nothing_of(items):
    """the verdict is made of what staging left: with every converting window turned away mid-call the table is the existing kernel's"""
    case = DM.cases()[0]
    rc, before, _ = TD.call(items, case.windows, case.frames, case.channels, dense_flags=MIX)
    final = [int(r[1]) for r in before["report"]]
    conv = [k for k in range(len(final)) if final[k] and case.mode(k, False) == DM.DOWN]
    assert len(conv) > 10
    for k in conv[1:]:
        final[k] = 0
    rc, got, tot = TD.call(items, case.windows, case.frames, case.channels, dense_flags=MIX, final_words=final)
    want = DM.model(items, case.windows, case.frames, case.channels, False, capi.PARSE_HOST, False, final_words=final)
    assert rc == 0 and TD.signed(got["rows"]) == want["rows"] and flat(got["mix"]) == want["mix"] and want["mix"][-1] == 1
    final[conv[0]] = 0
    rc, got, tot = TD.call(items, case.windows, case.frames, case.channels, dense_flags=MIX, final_words=final)
    assert rc == 0 and flat(got["mix"])[-1] == 0 and all(word >> DM.MODE_SHIFT == 0 for _, word in TD.signed(got["rows"]))
    assert flat(got["mix"])[:-1] == want["mix"][:-1]


def test_refusals_and_acceptances(items):
    """with the flag a window of an item that has a channel count is checked in that item's own frames; one without is checked against C"""
    wins, T = [(0, 8, 32), (2, 16, 64)], 64
    rc, tables, tot = TD.call(items, wins, frames=T, channels=1, dense_flags=MIX)
    assert rc == 0 and tot["out_words"] == 2 * T
    refused = (
        ("odd first_word on a stereo item, C = 1", (1, 3, 8), 1),
        ("odd max_words on a stereo item, C = 1", (1, 4, 7), 1),
        ("odd first_word of a stereo window that asks for nothing", (3, 1, 0), 1),
        ("max_words > 2T on a stereo item, C = 1", (1, 0, 2 * T + 2), 1),
        ("max_words > T on a mono item, C = 2", (0, 0, T + 1), 2),
        ("max_words > T on a mono item, C = 1", (0, 0, T + 1), 1),
        ("max_words > 2T on a stereo item, C = 2", (1, 0, 2 * T + 2), 2),
        ("odd first_word on a stereo item, C = 2", (1, 3, 8), 2),
        ("max_words > C * T on a blob that is not ACM", (7, 0, T + 1), 1),
        ("odd first_word on a blob that is not ACM, C = 2", (7, 3, 8), 2),
        ("odd max_words of no file at all, C = 2", (99, 0, 7), 2),
    )
    for what, bad, ch in refused:
        for planar in (0, 1):
            rc, tables, tot = TD.call(items, wins[:1] + [bad] + wins[1:], frames=T, channels=ch, dense_flags=MIX | planar)
            assert rc == capi.ERR_ARG and list(tables) == ["totals"], what
    accepted = (
        ("2T samples of a stereo item, C = 1", (1, 2, 2 * T), 1),
        ("exactly T samples of a mono item, C = 2", (0, 3, T), 2),
        ("an odd first_word and an odd count on a mono item, C = 2", (2, 5, 7), 2),
        ("2T samples of a blob that is not ACM, C = 2", (7, 0, 2 * T), 2),
    )
    for what, good, ch in accepted:
        for planar in (0, 1):
            rc, tables, tot = TD.call(items, wins[:1] + [good] + wins[1:], frames=T, channels=ch, dense_flags=MIX | planar, f32=bool(planar))
            assert rc == 0 and "mix" in tables, what
    # what the flag does not change: the other refusals of the call, an unknown flag beside it, no windows at all
    assert TD.call(items, wins, frames=T, channels=1, dense_flags=MIX | 2)[0] == capi.ERR_ARG
    assert TD.call(items, wins, frames=T, channels=1, dense_flags=MIX | 8)[0] == capi.ERR_ARG
    assert TD.call(items, wins, frames=T, channels=1, dense_flags=MIX, d_pcm_words=2 * T - 1)[0] == capi.ERR_ARG
    assert TD.call(items, wins, frames=T, channels=3, dense_flags=MIX, d_pcm_words=1000)[0] == capi.ERR_ARG
    # a row's record keeps its mode above 56 bits of count: longer rows are not taken with the flag
    assert TD.call(items, [], frames=1 << 55, channels=1, dense_flags=MIX, d_pcm_words=0)[0] == capi.ERR_ARG
    assert TD.call(items, [], frames=(1 << 55) - 1, channels=1, dense_flags=MIX, d_pcm_words=0)[0] == 0
    rc, tables, tot = TD.call(items, [], frames=T, channels=2, dense_flags=MIX)
    assert rc == 0 and list(tables) == ["mix", "totals"] and flat(tables["mix"]) == [0] and tot["table_bytes"] == 0


def test_calls_without_the_flag_are_untouched(items):
    """every dense_crops case without ACM_DENSE_MIX: the tables of the model that knows no such flag, window for window, and no other"""
    for case in DC.cases():
        for planar in (False, True):
            for parse in (capi.PARSE_HOST, capi.PARSE_DEVICE):
                rc, got, tot = TD.call(items, case.windows, case.frames, case.channels, dense_flags=int(planar), parse=parse)
                want = TD.model(items, case.windows, case.frames, case.channels, planar, parse, False)
                assert rc == 0 and list(got) == PLAIN_TABLES and tot == want["totals"], case.name
                assert TD.signed(got["wins"]) == want["wins"] and flat(got["rejected"]) == want["rejected"] and any(want["rejected"])
                assert TD.signed(got["report"]) == want["report"] and TD.signed(got["rows"]) == want["rows"]
                assert all(word >> DM.MODE_SHIFT == 0 for _, word in TD.signed(got["rows"]))


def test_the_flag_over_one_channel_count_changes_nothing(items):
    """all windows of the batch's own channel count (or of none): byte for byte the tables of the call without the flag, and the
    verdict is the existing kernel"""
    for case in DC.cases():
        wins = [w for k, w in enumerate(case.windows) if not case.rejected(k)]
        assert len(wins) > 20
        for planar in (False, True):
            for parse in (capi.PARSE_HOST, capi.PARSE_DEVICE):
                rc0, plain, tot0 = TD.call(items, wins, case.frames, case.channels, dense_flags=int(planar), parse=parse, f32=planar)
                rc1, mixed, tot1 = TD.call(items, wins, case.frames, case.channels, dense_flags=MIX | int(planar), parse=parse, f32=planar)
                assert rc0 == rc1 == 0 and tot0 == tot1 and list(mixed) == PLAIN_TABLES[:-1] + ["mix", "totals"]
                for name in PLAIN_TABLES:
                    assert plain[name].tobytes() == mixed[name].tobytes(), (case.name, name)
                assert flat(mixed["mix"]) == [DM.SPLIT if planar and case.channels == 2 else DM.COPY] * len(wins) + [0]


# ---------------------------------------------------------------------------------------------------------------- the case list

def test_case_list_reaches_what_the_kernel_can_get_wrong():
    cases = DM.cases()
    assert sorted((c.channels, c.frames) for c in cases) == [(1, 37), (1, 64), (2, 37), (2, 64)]
    kinds, levels = set(), set()
    residues = {DM.DOWN: set(), DM.UP_INTER: set(), DM.COPY: set()}
    for c in cases:
        lengths = {DM.COPY: set(), DM.DOWN: set(), DM.UP_INTER: set()}
        modes = [c.mode(k, False) for k in range(len(c.windows))]
        assert {DM.COPY, DM.DOWN if c.channels == 1 else DM.UP_INTER} == set(modes)
        assert {c.mode(k, True) for k in range(len(c.windows))} == ({DM.COPY, DM.DOWN} if c.channels == 1 else {DM.SPLIT, DM.UP_PLANAR})
        # consecutive rows alternate modes: more changes of mode than rows of the rarer one
        changes = sum(a != b for a, b in zip(modes, modes[1:]))
        assert changes >= min(modes.count(m) for m in set(modes)) and 2 * changes >= len(modes), (c.name, changes, len(modes))
        seen_files = set()
        for k, (f, first, count) in enumerate(c.windows):
            words, frames = c.delivers(k), c.frames_delivered(k)
            if f >= len(DC.files()):
                kinds.add("no such file")
                continue
            src = DC.files()[f]
            seen_files.add(f)
            if not src.acm:
                kinds.add("not ACM")
                continue
            assert first % src.channels == 0 and count % src.channels == 0 and count <= c.frames * src.channels
            converts = modes[k] != DM.COPY
            lengths[modes[k]].add(frames)
            if first >= src.words:
                kinds.add(("behind the end", converts))
            elif words < count:
                kinds.add(("clipped by the end" if src.end_status == 0 else "clipped by a stream that breaks off", converts))
            if frames >= 9:
                residues[modes[k]].add(first % 8)
                levels.add((src.info.level, src.channels, converts))
            if words and first // src.st.block_len != (first + words - 1) // src.st.block_len:
                kinds.add(("across a block boundary", converts))
        assert seen_files == set(range(8)), c.name
        for mode, got in lengths.items():
            if mode in modes:
                assert {0, 1, 7, 8, 9, c.frames - 1, c.frames} <= got, (c.name, mode, sorted(got))
    assert residues[DM.DOWN] == {0, 2, 4, 6} and residues[DM.UP_INTER] == set(range(8)) and residues[DM.COPY] == set(range(8))
    both = {(what, conv) for what in ("behind the end", "clipped by the end", "across a block boundary") for conv in (False, True)}
    # the file that breaks off is mono: plain in a mono batch, up-mixed in a stereo one
    assert kinds == both | {"no such file", "not ACM", ("clipped by a stream that breaks off", False), ("clipped by a stream that breaks off", True)}
    assert levels == {(lv, ch, conv) for lv in (1, 5, 9) for ch in (1, 2) for conv in (False, True)}, sorted(levels)


def test_up_mixed_bodies_start_on_either_copy_of_a_sample(items):
    """the body of an up-mixed interleaved row starts on the first copy of a sample in the buffers of test_expected_rows and on the
    second one in those of test_interleaved_stereo_batch_one_element_off_a_line (DM.ODD_SHIFT), int16 and float32; either way the rows
    with at least one whole 16-output vector read their source at every residue modulo 8 samples"""
    for case in DM.cases():
        if case.channels != 2:
            continue
        rc, got, tot = TD.call(items, case.windows, case.frames, 2, dense_flags=MIX)
        rows = TD.signed(got["rows"])
        for shift, parity in ((0, 0), (DM.ODD_SHIFT, 1)):
            for unit in (2, 4):
                residues = set()
                for k, (src, word) in enumerate(rows):
                    head = DM.head_of(k, case.row, unit, shift)
                    assert head % 2 == parity and head < 8, (case.name, unit, shift, k, head)
                    if word >> DM.MODE_SHIFT == DM.UP_INTER and 2 * (word & ((1 << DM.MODE_SHIFT) - 1)) >= head + 16:
                        residues.add((src + head // 2) % 8)
                assert residues == set(range(8)), (case.name, unit, shift, sorted(residues))


def test_down_mixed_frames_tell_the_laws_apart():
    """among the frames the mono cases deliver from stereo files: an odd negative sum (floor and truncation differ), an odd positive
    one, a sum beyond int16 (a 16-bit sum would wrap) - from every stereo file"""
    assert [int(DM.sums(f).size) for f in (1, 3, 5)] == [240, 747, 1897]
    for c in DM.cases():
        if c.channels != 1:
            continue
        seen = {f: dict.fromkeys(DM.SUM_KINDS, 0) for f in (1, 3, 5)}
        for k, (f, first, count) in enumerate(c.windows):
            if c.mode(k, False) == DM.DOWN and c.delivers(k):
                s = DM.sums(f)[first // 2:first // 2 + c.frames_delivered(k)]
                for what, kind in DM.SUM_KINDS.items():
                    seen[f][what] += int(kind(s).sum())
        assert all(n > 0 for per_file in seen.values() for n in per_file.values()), (c.name, seen)


def test_expected_rows_follow_the_formula():
    """the builder's vectorised rows against the contract's table spelled out element by element, on a sample of each case that holds
    every mode"""
    rng = np.random.default_rng(0xD1)
    for c in DM.cases():
        C, T = c.channels, c.frames
        for planar in (False, True):
            rows = c.rows(planar)
            assert rows.shape == (len(c.windows), c.row) and rows.any()
            picked = set(rng.choice(len(c.windows), 16, replace=False).tolist())
            assert {c.mode(k, planar) for k in picked} == {c.mode(k, planar) for k in range(len(c.windows))}
            for k in picked:
                f, first, count = c.windows[k]
                ck = DM.chans_of(f, C)
                fr = c.delivers(k) // ck
                whole = DC.files()[f].pcm.tolist() if f < len(DC.files()) else []
                for e in range(c.row):
                    i, ch = (e % T, e // T) if planar else (e // C, e % C)          # output frame and channel of element e
                    if i >= fr:
                        want = 0
                    elif ck == C:
                        want = whole[first + i * ck + ch]
                    elif C == 1:
                        want = (whole[first + 2 * i] + whole[first + 2 * i + 1]) >> 1
                    else:
                        want = whole[first + i]
                    assert rows[k, e] == want, (c.name, planar, k, e)
    # the law itself, on the values the contract names (Python's >> on its unbounded integers is the arithmetic shift)
    assert (32767 + 32767) >> 1 == 32767 and (-1 + 0) >> 1 == -1 and (-32768 - 32768) >> 1 == -32768 and (-3 + 0) >> 1 == -2


# ---------------------------------------------------------------------------------------------------------------- the kernel's code

@pytest.fixture(scope="module")
def kernel_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "acm_dense_mix.s"
    cmd = [_build.HIPCC, "-O3", "-std=c++17", "--offload-arch=" + _build.GFX, "-I", _build.INC, "-I", _build.CSRC,
           "--cuda-device-only", "-S", "-o", str(out), os.path.join(_build.CSRC, "acm_dense_mix.hip")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return out.read_text()


def test_kernel_has_wide_accesses_and_no_scratch(kernel_asm):
    """all six builds ({int16, float32} x {mono, interleaved stereo, planar stereo}), each with the bodies of its two modes: 16-byte
    global loads and stores - at least one load and one store (two of float32) per mode - no flat, buffer, scratch or LDS access, no
    private segment, no group segment; nothing in the file is called acm_dense_rows"""
    assert "acm_dense_rows" not in kernel_asm
    bodies = {}
    for m in re.finditer(r"^(_ZN\S*acm_dense_mixed\S*):", kernel_asm, re.M):
        bodies[m.group(1)] = kernel_asm[m.end():kernel_asm.index(".Lfunc_end", m.end())]
    assert len(bodies) == 6, sorted(bodies)
    for name, body in bodies.items():
        ops = re.findall(r"^\s+((?:global|flat|scratch|buffer|ds)_\w+)", body, re.M)
        f32 = "mixedIf" in name
        assert ops.count("global_load_dwordx4") >= 2, (name, ops)
        assert ops.count("global_store_dwordx4") >= (4 if f32 else 2), (name, ops)
        assert not [o for o in ops if o.startswith(("flat_", "scratch_", "buffer_", "ds_"))], (name, ops)
        # narrow accesses are the head, the tail and the vector a short row ends in: 16-bit loads (a frame's two as one dword); 2- or
        # 4-byte stores
        assert set(ops) <= {"global_load_dwordx4", "global_store_dwordx4", "global_load_sshort", "global_load_ushort", "global_load_short_d16",
                            "global_load_short_d16_hi", "global_load_dword", "global_store_short", "global_store_dword"}, (name, sorted(set(ops)))
        meta = re.search(r"\.name:\s+%s\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)" % re.escape(name), kernel_asm)
        assert meta and int(meta.group(1)) == 0, name
        desc = kernel_asm[kernel_asm.index(".amdhsa_kernel " + name):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc) and re.search(r"\.amdhsa_group_segment_fixed_size 0\b", desc), name
