"""The crafted streams of tests/extreme_content.py through every kernel family, bit-exact against the CPU oracle.

What the streams are for: the matrix first pass of acm_chunk and of acm_tile2's matrix builds is exact because every
plane sum stays below 2^18 - the aligned streams put it AT the bound the coefficients allow (+232 353 / -232 257 for a byte plane of
the six-stage pass; tests/test_extreme_content.py derives and asserts the figures), with header values 0, 1, 255, 65535 and the
border of the one-instruction join around them; the constant and checker streams sit on the ends of every width class (the row sums
of the whole-range correction, the packed form's 0-bit residual with a non-zero base), the border streams on the borders between the
classes, the impulse streams put one extreme index where a wrong carry, history or lead-in shows as a local difference.

One plan per test over all of a level's streams; the PCM arena is poisoned before every launch and what lies between the streams must
keep the poison.  Files, staged forms and the oracle's PCM are made once per level and shared."""
import functools

import numpy as np
import pytest

import extreme_content as X
import helpers  # noqa: F401  (GPU tests run with the fill mode on: helpers sets the switch)
from libacm_amd import capi
from test_gpu_pcm_f32 import f32_bits, run_f32

pytestmark = pytest.mark.gpu

FORM_LEVELS = [7, 8, 9, 10, 11, 12, 13, 14]
GENERAL_LEVELS = [0, 1, 2, 3, 4, 5, 7, 9, 12, 13, 15]          # (0-4: constant, checker and impulse streams only - no matrix pass there)
POISON = 0xA5


@functools.lru_cache(None)
def staged(level):
    return [capi.stage_file(s.data) for s in X.level_streams(level)]


def say(level, k, got, want):
    bad = np.nonzero(got != want)[0]
    cols = 1 << level
    return "level %d stream %d (%s): %d of %d samples differ, first at %d = row %d column %d" % (
        level, k, X.level_streams(level)[k].name, bad.size, want.size, bad[0], bad[0] // cols, bad[0] % cols)


def decode(dev, level, flags, form="int16", unbind=False, first_row=0):
    """one plan over every crafted stream of the level.  form: "int16", "byteplane" or "packed" (the second staged form bound);
    unbind: the plan is cut with the byte-plane form and launched without it (the int16 twins of its records); first_row: every
    stream as a window from that row on (the form is that of the whole streams)"""
    st = staged(level)
    want = X.level_oracle(level)
    cols = 1 << level
    ar = capi.Arena(st, [(first_row, s.words - first_row * cols) for s in st] if first_row else None)
    ptrs = [dev.malloc(ar.idx.nbytes), dev.malloc(ar.hdr.nbytes), dev.malloc(ar.pcm_words * 2)]
    d_idx, d_hdr, d_pcm = ptrs
    try:
        dev.upload(d_idx, ar.idx)
        dev.upload(d_hdr, ar.hdr)
        assert ar.patches is None
        pk = None
        if form == "byteplane":
            whole = capi.Arena(st).descs if first_row else ar.descs            # (same idx / hdr offsets: they do not depend on the windows)
            pk = capi.mform_streams(ar.idx, whole)
        elif form == "packed":
            pk = capi.pack_streams(ar.idx, ar.descs)
        if pk:
            ptrs += pk.upload(dev)
        plan = capi.Plan(dev, ar.descs, None, flags, packed=pk.streams if pk else None)
        if form == "byteplane":
            plan.bind_mform(*((None, None) if unbind else ptrs[3:]))
        elif form == "packed":
            plan.bind_packed(*ptrs[3:])
        stats = plan.stats()
        dev.memset(d_pcm, POISON, ar.pcm_words * 2)
        plan.launch(d_idx, d_hdr, d_pcm)
        out = np.empty(ar.pcm_words, dtype=np.uint16)
        dev.download(out, d_pcm)
        plan.destroy()
    finally:
        for p in ptrs:
            dev.free(p)
    written = np.zeros(ar.pcm_words, bool)
    for k, (d, (pcm, _)) in enumerate(zip(ar.descs, want)):
        ref = pcm[first_row * cols:]
        assert d.n_emit == ref.size
        got = out[d.pcm_off:d.pcm_off + d.n_emit]
        assert np.array_equal(got, ref), say(level, k, got, ref)
        written[d.pcm_off:d.pcm_off + d.n_emit] = True
    assert (out[~written] == POISON * 0x101).all(), "PCM written outside the streams' samples"
    return stats


@pytest.mark.parametrize("level", FORM_LEVELS)
@pytest.mark.parametrize("unbind", [False, True], ids=["form", "int16_twins"])
def test_matrix_first_pass_on_the_byteplane_form(dev, level, unbind):
    """ACMHIP_PLAN_LEAN_ALWAYS with the byte-plane form: acm_chunk at levels 8-12 (fast path at 8, 12 and 16 bits in the streams of tall
    blocks, the general path with its differences of row values 0 <-> 65535 in those of one- and three-row blocks, the whole-range
    class), the matrix builds of acm_tile2 at 7, 13 and 14; and the same plan sent back to the int16 arena (acmhip_plan_bind_mform(NULL))"""
    stats = decode(dev, level, capi.PLAN_LEAN_ALWAYS, "byteplane", unbind=unbind)
    assert stats.mform_tiles >= 4 * len(staged(level))
    assert stats.fused_streams == len(staged(level)) and stats.stagewise_streams == 0


@pytest.mark.parametrize("level", [6] + FORM_LEVELS)
def test_lean_kernels_on_the_int16_form(dev, level):
    """ACMHIP_PLAN_LEAN_ALWAYS without a second form: acm_tile2's vector-ALU build reads the int16 rows"""
    stats = decode(dev, level, capi.PLAN_LEAN_ALWAYS)
    assert stats.mform_tiles == 0 and stats.stagewise_streams == 0


@pytest.mark.parametrize("level", GENERAL_LEVELS)
@pytest.mark.parametrize("flags", [capi.PLAN_NO_LEAN | capi.PLAN_FORCE_HALO, capi.PLAN_NO_LEAN | capi.PLAN_FORCE_CARRY, capi.PLAN_STAGEWISE],
                         ids=["halo", "carry", "stagewise"])
def test_general_and_stagewise_kernels(dev, level, flags):
    """no lean kernel: acm_small_level (levels 0-4), acm_fused_tile in its halo and carry builds (5-12), the prefix sweep and the plane
    build (13-15); and unpack + one launch per stage (ACMHIP_PLAN_STAGEWISE)"""
    stats = decode(dev, level, flags)
    if flags == capi.PLAN_STAGEWISE:
        assert stats.stagewise_streams == len(staged(level))
    else:
        assert stats.stagewise_streams == 0 and stats.mform_tiles == 0


@pytest.mark.parametrize("level", [6, 7, 8, 9])
def test_packed_form(dev, level):
    """acm_tile2p: the constant streams are 0-bit residuals on a base at the end of the range, the border streams change the width of
    a column pair's group for one index"""
    stats = decode(dev, level, capi.PLAN_LEAN_ALWAYS, "packed")
    assert stats.packed_tiles >= 4 * len(staged(level))


@pytest.mark.parametrize("level", FORM_LEVELS)
@pytest.mark.parametrize("form", ["byteplane", "int16"])
def test_float_output(dev, level, form):
    """acmhip_plan_launch_f32 of the lean kernels: the float twins of the matrix first pass (and of the vector-ALU build) write the
    s16le sample times 2^-15, exactly"""
    stats = run_f32(dev, [s.data for s in X.level_streams(level)], flags=capi.PLAN_LEAN_ALWAYS, form=form)
    assert (stats.mform_tiles > 0) == (form == "byteplane")


@pytest.mark.parametrize("level", [8, 9, 10, 11, 12])
def test_windows_replay_aligned_rows(dev, level):
    """every stream as a window from its third tile on, on the byte-plane form: the lead-in chunk (ACM_TILE_DISCARD) decodes the aligned
    rows in front of the window for their carries and stores them into the sink"""
    t2 = capi.lib().acmk_tile2_rows(level)
    stats = decode(dev, level, capi.PLAN_LEAN_ALWAYS, "byteplane", first_row=2 * t2)
    assert stats.mform_tiles >= 2 * len(staged(level))


@functools.lru_cache(None)
def batch():
    """the crafted files of every level, side by side, and the oracle's PCM for them"""
    files, want = [], []
    for level in range(16):
        files += [s.data for s in X.level_streams(level)]
        want += [pcm for pcm, _ in X.level_oracle(level)]
    return files, want


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("staging", [capi.BATCH_STAGE_BYTEPLANE, capi.BATCH_STAGE_INT16], ids=["byteplane", "int16"])
@pytest.mark.parametrize("parse,ranges", [(capi.PARSE_HOST, 0), (capi.PARSE_DEVICE, 1), (capi.PARSE_DEVICE, 3)], ids=["host", "device", "device_3_ranges"])
def test_batch_decode(dev, parse, ranges, staging, f32):
    """acm_batch_decode over every level's crafted files at once: bits parsed on the host pool and on the device (in one piece and in
    three block ranges), byte-plane and int16 staging, int16 and float32 PCM.  (The device parser takes a block's width class from its
    pwr alone: what the host stager stores at 12 bits travels at 16 bits there.)"""
    files, want = batch()
    cap = capi.batch_pcm_words(files)
    size = 4 if f32 else 2
    d_pcm = dev.malloc(cap * size)
    try:
        dev.memset(d_pcm, 0xFF if f32 else POISON, cap * size)
        status, words, offs, tm = capi.batch_decode_device(dev, files, d_pcm, cap, threads=8, parse=parse, f32=f32,
                                                           batch_flags=staging | (capi.batch_ranges(ranges) if ranges else 0))
        out = np.empty(cap, np.uint32 if f32 else np.uint16)
        dev.download(out, d_pcm)
    finally:
        dev.free(d_pcm)
    assert (tm.device_parsed > 0) == (parse == capi.PARSE_DEVICE)
    assert (tm.packed_streams > 0) == (staging == capi.BATCH_STAGE_BYTEPLANE)
    written = np.zeros(cap, bool)
    for k, (pcm, a, n) in enumerate(zip(want, offs, words)):
        assert status[k] == 0 and n == pcm.size, k
        ref = f32_bits(pcm) if f32 else pcm
        assert np.array_equal(out[a:a + n], ref), "file %d: %d samples differ, first at %d" % (k, (out[a:a + n] != ref).sum(), np.nonzero(out[a:a + n] != ref)[0][0])
        written[a:a + n] = True
    assert (out[~written] == (0xFFFFFFFF if f32 else POISON * 0x101)).all()
