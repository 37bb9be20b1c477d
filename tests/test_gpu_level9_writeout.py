"""Level 9's write-out on a byte boundary (libacm_amd/csrc/acm_late_scale.h): byte for byte against the CPU oracle at the
smallest shapes that reach every level-9 kernel whose write-out ends in lds_pass, in every sample format and as float32.

The streams: tests/extreme_content.py's aligned content of the 16-bit class at the output where the six-stage bound is attained
(+232 353 / -232 257 per plane), both signs, under header values 0, 1, 255 and 65535 - products past 2^24, where bit 24 and what lies
above it are NOT a sign extension, which is what a wrong shift or a bit lost between the injecting stage and the exact one gets wrong -
in blocks of 1 row (five blocks: a stream's first chunk takes `fresh` and the zeroed carry, the fifth row the general kernel), of 3
rows (five blocks) and of 16 rows (four blocks = 16 chunks of the chunk kernel in one run, four tiles of acm_tile2: chunk and tile
boundaries cross the scaled history of the last stage), and one stream of random indices.

One plan per test over all of them, the PCM arena poisoned before the launch; streams, staged forms and the oracle's PCM are made once."""
import functools

import numpy as np
import pytest

import extreme_content as X
import helpers
from helpers import crafted_stream, make_stream, oracle_pcm
from libacm_amd import capi
from test_gpu_pcm_f32 import f32_bits

pytestmark = pytest.mark.gpu

LEVEL = 9
VALS = [65535, 0, 1, 255]
FORMATS = [capi.FMT_S16LE, capi.FMT_S16BE, capi.FMT_U16LE, capi.FMT_U16BE, "f32"]
FORMAT_IDS = ["s16le", "s16be", "u16le", "u16be", "f32"]


def aligned_stream(height, nblocks, signs, first_val, cut):
    q = X.bound_outputs(X.stages(LEVEL))[0]
    idx, meta = X.aligned(LEVEL, X.CLS16, q, signs[0], signs[1], height * nblocks)
    blocks = []
    for b in range(nblocks):
        rows = idx[b * height:(b + 1) * height]
        code = X._code(rows)
        blocks.append((code - 1, VALS[(b + first_val) % len(VALS)], code, rows))
    return crafted_stream(LEVEL, height, blocks, cut=cut)


@functools.lru_cache(None)
def streams():
    out = [aligned_stream(1, 5, "++", 0, 3), aligned_stream(1, 5, "--", 3, 0),
           aligned_stream(3, 5, "++", 2, 1), aligned_stream(3, 5, "--", 0, 5),
           aligned_stream(16, 4, "++", 3, 7), aligned_stream(16, 4, "--", 0, 0),
           make_stream(9900, LEVEL, 16, 3, cut=11, val_max=65535, pwr_max=15)]
    return out


@functools.lru_cache(None)
def staged():
    return [capi.stage_file(f) for f in streams()]


@functools.lru_cache(None)
def oracle(fmt):
    """per stream the oracle's samples in this format, as the words the arena must hold (float32: the bits of s16le * 2^-15)"""
    be, sgned = (0, 1) if fmt == "f32" else helpers.fmt_args(fmt)
    out = []
    for f in streams():
        pcm, _ = oracle_pcm(f, be=be, sgned=sgned)
        pcm = f32_bits(pcm) if fmt == "f32" else pcm
        pcm.flags.writeable = False
        out.append(pcm)
    return out


def test_content_attains_the_bound():
    """(no device) the aligned streams are what the docstring says: a plane sum at the bound on both signs, times 65535 past 2^24"""
    G = X.stages(LEVEL)
    q = X.bound_outputs(G)[0]
    for signs, want in (("++", X.bounds(G, X.BYTE)[0][q]), ("--", X.bounds(G, X.BYTE)[1][q])):
        idx, _ = X.aligned(LEVEL, X.CLS16, q, signs[0], signs[1], 6)
        lo, hi = X.planes(X.CLS16, idx)
        assert any(X.first_stages(p, 1 << LEVEL, G).reshape(6, -1)[2:].__abs__().max() == abs(want) for p in (lo, hi))
    assert int(X.bounds(G, X.BYTE)[0][q]) == 232353 and int(X.bounds(G, X.BYTE)[1][q]) == -232257
    assert 232353 * 65535 > 1 << 24


def decode(dev, fmt, flags, form="int16", windows=None):
    st = staged()
    f32 = fmt == "f32"
    cols = 1 << LEVEL
    ar = capi.Arena(st, windows)
    size = 4 if f32 else 2
    ptrs = [dev.malloc(ar.idx.nbytes), dev.malloc(ar.hdr.nbytes), dev.malloc(ar.pcm_words * size)]
    d_idx, d_hdr, d_pcm = ptrs
    try:
        dev.upload(d_idx, ar.idx)
        dev.upload(d_hdr, ar.hdr)
        assert ar.patches is None
        pk = None
        if form == "byteplane":
            pk = capi.mform_streams(ar.idx, capi.Arena(st).descs)        # the form of the whole streams (same idx / hdr offsets)
        elif form == "packed":
            pk = capi.pack_streams(ar.idx, ar.descs)
        if pk:
            ptrs += pk.upload(dev)
        plan = capi.Plan(dev, ar.descs, None, flags, packed=pk.streams if pk else None)
        if form == "byteplane":
            plan.bind_mform(*ptrs[3:])
        elif form == "packed":
            plan.bind_packed(*ptrs[3:])
        stats = plan.stats()
        helpers.poison_pcm(dev, d_pcm, ar.pcm_words, f32)
        if f32:
            plan.launch_f32(d_idx, d_hdr, d_pcm)
        else:
            plan.launch(d_idx, d_hdr, d_pcm, fmt)
        out = np.empty(ar.pcm_words, dtype=np.uint32 if f32 else np.uint16)
        dev.download(out, d_pcm)
        plan.destroy()
    finally:
        for p in ptrs:
            dev.free(p)
    written = np.zeros(ar.pcm_words, bool)
    for k, (d, pcm) in enumerate(zip(ar.descs, oracle(fmt))):
        ref = pcm[d.row_begin * cols:d.row_begin * cols + d.n_emit]
        assert ref.size == d.n_emit
        got = out[d.pcm_off:d.pcm_off + d.n_emit]
        bad = np.nonzero(got != ref)[0]
        assert bad.size == 0, "stream %d: %d of %d samples differ, first at row %d column %d: %#x for %#x" % (
            k, bad.size, ref.size, d.row_begin + bad[0] // cols, bad[0] % cols, got[bad[0]], ref[bad[0]])
        written[d.pcm_off:d.pcm_off + d.n_emit] = True
    assert (out[~written] == (0xFFFFFFFF if f32 else 0xA5A5)).all(), "PCM written outside the streams' samples"
    return stats


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_chunk_kernel(dev, fmt):
    """the byte-plane form: acm_chunk<9> (its float twin), 16 chunks in the runs of the tall streams, the fast path under header values
    1 and 255 and the general one where 0 and 65535 meet inside a chunk's reach; the ragged rows go to the general kernel"""
    stats = decode(dev, fmt, capi.PLAN_LEAN_ALWAYS, "byteplane")
    assert stats.mform_tiles >= 2 * 15               # the tall streams alone: 16 whole chunks, and 15 where the last one is cut


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_chunk_kernel_window_with_a_lead_in(dev, fmt):
    """the tall streams as windows from their second tile on: the chunk in front is replayed into the sink for its carries - the last
    stage's history arrives in scaled units from a chunk whose samples nobody keeps"""
    t2 = capi.lib().acmk_tile2_rows(LEVEL)
    cols = 1 << LEVEL
    wins = [(t2, s.words - t2 * cols) if s.info.blocks * s.info.rows >= 3 * t2 else (0, s.words) for s in staged()]
    assert sum(1 for w in wins if w[0]) >= 3
    stats = decode(dev, fmt, capi.PLAN_LEAN_ALWAYS, "byteplane", windows=wins)
    assert stats.mform_tiles >= 2 * 11


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_tile_kernel_on_the_int16_form(dev, fmt):
    """acm_tile2<9> (vector-ALU first pass; its float twin) takes the whole tiles, acm_fused_tile the streams shorter than one"""
    stats = decode(dev, fmt, capi.PLAN_LEAN_ALWAYS)
    assert stats.mform_tiles == 0 and stats.tiles >= 2 * 3 and stats.stagewise_streams == 0


@pytest.mark.parametrize("fmt", FORMATS[:4], ids=FORMAT_IDS[:4])
def test_packed_build(dev, fmt):
    """acm_tile2p<9>: every stage an LDS pass (the packed form has no float32 build)"""
    stats = decode(dev, fmt, capi.PLAN_LEAN_ALWAYS, "packed")
    assert stats.packed_tiles >= 2 * 3


@pytest.mark.parametrize("flags", [capi.PLAN_NO_LEAN | capi.PLAN_FORCE_HALO, capi.PLAN_NO_LEAN | capi.PLAN_FORCE_CARRY], ids=["halo", "carry"])
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_general_tile_kernel(dev, fmt, flags):
    """acm_fused_tile at level 9 ends in lds_pass too, in its halo and in its carry build"""
    stats = decode(dev, fmt, flags)
    assert stats.mform_tiles == 0 and stats.stagewise_streams == 0
