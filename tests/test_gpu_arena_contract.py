"""The kernels' arena contract (include/acm_hip.h) on the GPU: 8-word offsets, ragged counts, guards.

Every kernel family a plan can pick is forced in turn over the arenas of tests/arena_contract.py: idx_off and pcm_off on every residue of
8 words modulo 64, header runs behind poison headers, the staged rows surrounded by index 0x7FFF, n_emit of every residue modulo 8
around a row, a tile and the end of the stream, windows from rows 1, 2, T and T + 1.  Each plan is launched in the four 16-bit formats and
in float32 (the packed form has no float build), each launch into a freshly poisoned arena; every slot must be the oracle's slice, bit
for bit, and every word outside [pcm_off, pcm_off + n_emit) of the slots must keep the poison.  plan.stats() shows that the family the
case is about took the work.

The batch front end lays out its own arena (acm_batch_decode with device-resident output): the same "nothing outside
[dev_off, dev_off + words)" for int16, for files that end 1 to 7 samples short of a block, a truncated one and one that is no ACM file.
The CPU half - the builder's properties, and the library's host synthesis on the same arenas - is tests/test_arena_contract.py."""
import numpy as np
import pytest

import arena_contract as AC
from helpers import fmt_args, make_stream, oracle_pcm
from libacm_amd import capi

pytestmark = pytest.mark.gpu

NO_LEAN_HALO = capi.PLAN_NO_LEAN | capi.PLAN_FORCE_HALO
NO_LEAN_CARRY = capi.PLAN_NO_LEAN | capi.PLAN_FORCE_CARRY
# name -> (plan flags, second staged form, levels)
CASES = {
    "stagewise": (capi.PLAN_STAGEWISE, None, range(16)),
    "halo": (NO_LEAN_HALO, None, range(16)),
    "carry": (NO_LEAN_CARRY, None, range(16)),
    "auto": (capi.PLAN_AUTO, None, range(6, 15)),
    "lean": (capi.PLAN_LEAN_ALWAYS, None, range(6, 15)),
    "byteplane": (capi.PLAN_LEAN_ALWAYS, "byteplane", range(7, 15)),
    "byteplane_unbound": (capi.PLAN_LEAN_ALWAYS, "byteplane", range(7, 15)),       # the int16 twins of the byte-plane records
    "packed": (capi.PLAN_LEAN_ALWAYS, "packed", range(6, 10)),
}
# level by level: the level's arenas and oracle decodes are built once (arena_contract.contract) and shared by its cases
MATRIX = [(level, name) for level in range(16) for name, (_, _, levels) in CASES.items() if level in levels]


def second_form(ct, form):
    """the byte-plane / packed form of every copy of every source, and per descriptor the PackedStream of the copy it reads (none for
    a source with H1 patches)"""
    whole, which = ct.whole_copy_descs()
    arena = capi.mform_streams(ct.idx, whole) if form == "byteplane" else capi.pack_streams(ct.idx, whole)
    streams = []
    for i, w in enumerate(which):
        p = arena.streams[w]
        patched = bool(ct.sources[ct.desc_source[i]].patches)
        streams.append(capi.PackedStream(p.chunk_off, 0 if patched else p.ntiles, p.form))
    return arena, streams


def lean_rows(ct, i, t2, windows):
    """rows of descriptor i that go to the lean kernels: its whole tiles, for a stream without patches that starts at row 0 - or
    (windows: the byte-plane form at levels up to 12) on a tile boundary"""
    d = ct.descs[i]
    if ct.sources[ct.desc_source[i]].patches or d.row_begin % t2 or (d.row_begin and not windows):
        return 0
    return min(d.nrows - d.row_begin, d.n_emit >> d.level) // t2 * t2


def check_stats(ct, name, plan, st):
    L = capi.lib()
    level, n = ct.level, len(ct.descs)
    patched = sum(1 for k in ct.desc_source if ct.sources[k].patches)
    assert st.samples == sum(d.n_emit for d in ct.descs)
    assert st.fused_streams + st.stagewise_streams == n
    if name == "stagewise":
        assert st.stagewise_streams == n and st.tiles == 0
        return
    if name in ("halo", "carry"):
        assert st.mform_tiles == 0 and st.packed_tiles == 0
        if level <= 4:          # the register kernel; a stream with H1 patches goes to the stage-wise kernels there
            assert st.tiles == 0 and st.stagewise_streams == patched and st.fused_streams == n - patched
        else:
            assert st.tiles > 0 and st.stagewise_streams == 0
        return
    t2 = L.acmk_tile2_rows(level)
    assert st.stagewise_streams == 0 and st.tiles > 0
    if name in ("auto", "lean"):
        assert st.mform_tiles == 0 and st.packed_tiles == 0
        return
    if name == "packed":
        assert st.mform_tiles == 0 and st.packed_tiles == sum(lean_rows(ct, i, t2, False) for i in range(n)) // t2 > 0
        return
    # the byte-plane form: whole tiles from row 0, and (levels up to 12) from a tile boundary, in tiles of the matrix build's height; a
    # window's records start with the lead-in chunks of the tile in front of it (ACM_TILE_DISCARD: decoded for their carries, stored
    # into the sink), which count as tiles as well
    tm = L.acmhip_mform_tile_rows(level)
    rows = [lean_rows(ct, i, t2, level <= 12) for i in range(n)]
    for i in range(n):
        assert plan.form_rows(i) == rows[i], ct.describe(i)
    lead = min(t2, tm * L.acmk_tile2m_lead_in(level)) // tm
    assert sum(rows) > 0 and any(r and ct.descs[i].row_begin for i, r in enumerate(rows)) == (level <= 12)
    assert st.mform_tiles == sum(r // tm + (lead if ct.descs[i].row_begin and r else 0) for i, r in enumerate(rows))


@pytest.mark.parametrize("level,name", MATRIX, ids=["%d-%s" % m for m in MATRIX])
def test_plan_keeps_the_contract(dev, level, name):
    flags, form, _ = CASES[name]
    ct = AC.contract(level)
    arena, streams = second_form(ct, form) if form else (None, None)
    d_idx, d_hdr, d_pcm = dev.malloc(ct.idx.nbytes), dev.malloc(ct.hdr.nbytes), dev.malloc(ct.pcm_words * 4)
    form_ptrs = arena.upload(dev) if arena else ()
    plan = None
    try:
        dev.upload(d_idx, ct.idx)
        dev.upload(d_hdr, ct.hdr)
        plan = capi.Plan(dev, ct.descs, ct.patches, flags, packed=streams)
        if form == "byteplane":
            plan.bind_mform(*form_ptrs)
            if name == "byteplane_unbound":
                plan.bind_mform(None, None)
        elif form == "packed":
            plan.bind_packed(*form_ptrs)
        check_stats(ct, name, plan, plan.stats())
        for fmt in AC.FORMATS + (() if form == "packed" else (AC.F32,)):
            got = ct.poisoned(fmt)
            dev.memset(d_pcm, 0xFF if fmt == AC.F32 else 0xA5, got.nbytes)
            if fmt == AC.F32:
                plan.launch_f32(d_idx, d_hdr, d_pcm)
            else:
                plan.launch(d_idx, d_hdr, d_pcm, fmt)
            got[:] = 0
            dev.download(got, d_pcm)
            ct.check(got, fmt, "level %d, %s:" % (level, name))
    finally:
        if plan is not None:
            plan.destroy()
        for p in (d_idx, d_hdr, d_pcm) + tuple(form_ptrs):
            dev.free(p)


# ---- the batch front end: its own arena -----------------------------------------------------------------------------------------------

def ragged_corpus():
    """files that end 1 to 7 samples short of their last block (levels 0-15, heights 1 / odd / 16), a truncated file, a file that is no
    ACM file"""
    files = []
    for k, level in enumerate((7, 9, 0, 3, 5, 6, 8, 10, 11, 12, 13, 14, 15, 4)):
        rows = (16, 5, 1, 3)[k % 4] if level < 13 else 1 + k % 2
        nb = max(2, min(40, (3 << 15 >> level) // rows + 1))
        files.append(make_stream(32000 + k, level, rows, nb, cut=1 + k % 7))
    files.append(files[0][:len(files[0]) * 2 // 3])
    files.append(b"not an acm file")
    return files


@pytest.mark.parametrize("parse,ranges", [(capi.PARSE_HOST, 0), (capi.PARSE_DEVICE, 1), (capi.PARSE_DEVICE, 3)])
def test_batch_int16_stays_inside_its_streams(dev, parse, ranges):
    """acm_batch_decode with device-resident int16 output into a poisoned arena: stream k is the oracle's PCM at
    [dev_off, dev_off + words) and not a word of the arena outside those ranges changes - host parsing, device parsing in one piece and
    in 3 block ranges, the four formats"""
    files = ragged_corpus()
    cap = capi.batch_pcm_words(files)
    d_pcm = dev.malloc(cap * 2)
    try:
        for fmt in AC.FORMATS:
            dev.memset(d_pcm, 0xA5, cap * 2)
            st, words, offs, tm = capi.batch_decode_device(dev, files, d_pcm, cap, fmt=fmt, threads=4, parse=parse,
                                                           batch_flags=capi.batch_ranges(ranges) if ranges else 0)
            got = np.zeros(cap, np.uint16)
            dev.download(got, d_pcm)
            assert st[-1] != 0 and st[-2] != 0 and words[-2] > 0 and all(s == 0 for s in st[:-2])
            if parse == capi.PARSE_DEVICE:
                assert tm.device_parsed > 0
            written = np.zeros(cap, bool)
            be, sg = fmt_args(fmt)
            for k, f in enumerate(files):
                a, b = offs[k], offs[k] + words[k]
                assert b <= cap and not written[a:b].any(), k
                written[a:b] = True
                if words[k]:
                    want = oracle_pcm(f, 0, be, sg)[0]
                    assert words[k] == want.size and np.array_equal(got[a:b], want), (k, fmt)
            dirty = np.nonzero(~written & (got != AC.POISON16))[0]
            if dirty.size:
                k = max((k for k in range(len(files)) if offs[k] <= dirty[0]), key=lambda k: offs[k])
                raise AssertionError("format %d: %d words written outside the streams; the first, word %d, lies %d words behind the end of stream %d "
                                     "(dev_off %d, words %d)" % (fmt, dirty.size, dirty[0], dirty[0] - offs[k] - words[k], k, offs[k], words[k]))
    finally:
        dev.free(d_pcm)
