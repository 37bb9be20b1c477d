"""The arena contract of include/acm_hip.h without a GPU: the builder of tests/arena_contract.py has the properties the GPU test
(tests/test_gpu_arena_contract.py) relies on, and the library's host synthesis keeps the contract on those arenas.

acmhip_host_synth / acmhip_host_synth_f32 take the same descriptor as a plan; the other host tests call them with idx_off = hdr_off =
pcm_off = 0.  Here every descriptor of every level runs on the contract arena with the arena's own offsets (8-word residues, headers
behind poison headers, ragged n_emit, windows), in the four 16-bit formats and in float32: every slot is the oracle's slice and every
word outside [pcm_off, pcm_off + n_emit) keeps its poison.  That the expectations come out right here is also what makes a failure of
the GPU test the kernels' and not the builder's.

The second half does the same for far_contract(level) and far_form(level, form), the contract at offsets past 32 bits
(tests/test_gpu_far_offsets.py): what is laid out where, that the boundaries are crossed by data some plan reads or writes, that the
aliases do not forgive, and that pieces, descriptors and expectations belong together."""
import numpy as np
import pytest

import arena_contract as AC
from libacm_amd import capi

LEVELS = list(range(16))


@pytest.mark.parametrize("level", LEVELS)
def test_builder_properties(level):
    ct = AC.contract(level)
    cols, T = ct.cols, ct.T
    assert len(ct.sources) == (3 if level in AC.H1_LEVELS else 2)
    for s in ct.sources:
        # the smallest whole-block shape with a whole tile, a second one and a ragged rest
        need = max(2 * T + 3, (2048 + cols - 1) // cols)
        assert need <= s.nrows < need + s.rows and s.nrows * cols >= 2048
        assert len(s.idx_off) == AC.COPIES
        assert bool(s.patches) == (s.name == "C")
    assert {d.idx_off % 64 for d in ct.descs} == set(range(0, 64, 8))
    assert {d.pcm_off % 64 for d in ct.descs} == set(range(0, 64, 8))
    assert {d.n_emit % 8 for d in ct.descs} == set(range(8))
    assert all(d.hdr_off > 0 for d in ct.descs) and {d.hdr_off % 2 for d in ct.descs} == {0, 1}
    assert all(AC.valid_desc(d) for d in ct.descs)
    assert {d.row_begin for d in ct.descs} == {0, 1, 2, T, T + 1}
    for k, s in enumerate(ct.sources):              # every copy of every source is read by some descriptor
        assert {c for kk, c in zip(ct.desc_source, ct.desc_copy) if kk == k} == set(range(AC.COPIES))
        assert sorted(o % 64 for o in s.idx_off) == sorted(AC.RESIDUES[k])
    # index arena: at least 8 words of poison in front of, between and behind the copies; header arena: poison in front of every run
    runs = sorted((o, o + s.nrows * cols) for s in ct.sources for o in s.idx_off)
    assert runs[0][0] >= 8 and ct.idx.size - runs[-1][1] >= 8
    assert all(b[0] - a[1] >= 8 for a, b in zip(runs, runs[1:]))
    assert (ct.idx[~ct.staged_words] == AC.IDX_POISON).all() and int(ct.staged_words.sum()) == sum(b - a for a, b in runs)
    hruns = sorted((o, o + s.st.info.blocks) for s in ct.sources for o in s.hdr_off)
    assert all(1 <= b[0] - a[1] <= 3 for a, b in zip([(0, 0)] + hruns, hruns))
    for o, _ in hruns:
        assert tuple(ct.hdr[o - 1]) == AC.HDR_POISON
    # PCM arena: slots in order, 8 to 71 words apart, 64 words behind the last; the mask is everything but the slots
    end = 0
    for k, d in enumerate(ct.descs):
        assert d.pcm_off % 64 == 8 * (k % 8) and 8 <= d.pcm_off - end < 8 + 64 + 8, k
        end = d.pcm_off + d.n_emit
        assert ct.mask[end:(end + 7) & ~7].all() and not ct.mask[d.pcm_off:end].any()
    assert ct.pcm_words == end + 64 and int((~ct.mask).sum()) == sum(d.n_emit for d in ct.descs)
    if ct.patches is not None:
        assert {p.stream for p in ct.patches} == {i for i, k in enumerate(ct.desc_source) if ct.sources[k].name == "C"}


def test_check_names_the_descriptor():
    """the failure messages of Contract.check: a word written behind a slot names the descriptor in front of it and the distance behind
    its n_emit; a wrong sample names its own slot"""
    ct = AC.contract(4)
    good = ct.expected_arena(capi.FMT_S16LE)
    ct.check(good.copy(), capi.FMT_S16LE)
    i = next(k for k, d in enumerate(ct.descs) if d.n_emit % 8 == 5)
    d = ct.descs[i]
    bad = good.copy()
    bad[d.pcm_off + d.n_emit + 2] = 1
    with pytest.raises(AssertionError, match=r"lies 2 words behind the n_emit of desc %d " % i):
        ct.check(bad, capi.FMT_S16LE)
    bad = good.copy()
    bad[d.pcm_off + 3] ^= 1
    with pytest.raises(AssertionError, match=r"the first is sample 3 of desc %d " % i):
        ct.check(bad, capi.FMT_S16LE)
    bad = good.copy()
    bad[5] = 0
    with pytest.raises(AssertionError, match="in front of the first slot"):
        ct.check(bad, capi.FMT_S16LE)


@pytest.mark.parametrize("fmt", list(AC.FORMATS) + [AC.F32])
@pytest.mark.parametrize("level", LEVELS)
def test_host_synth_keeps_the_contract(level, fmt):
    ct = AC.contract(level)
    ct.check(AC.host_launch(ct, fmt), fmt, "host synthesis")


def test_poison_indices_would_show():
    """the index poison is not inert: a read one word in front of a stream's staged rows changes the PCM (a descriptor whose idx_off
    is 8 words early decodes differently), so a kernel that reads outside the rows it was given cannot pass by luck"""
    ct = AC.contract(5)
    i = next(k for k, d in enumerate(ct.descs) if d.row_begin == 0 and d.n_emit == ct.cols + 3)
    d = capi.StreamDesc.from_buffer_copy(ct.descs[i])
    d.idx_off -= 8
    out = ct.poisoned(capi.FMT_S16LE)
    import ctypes as C
    assert capi.lib().acmhip_host_synth(C.byref(d), ct.idx.ctypes.data, ct.hdr.ctypes.data, None, 0, capi.FMT_S16LE, out.ctypes.data) == 0
    assert not np.array_equal(out[d.pcm_off:d.pcm_off + d.n_emit], ct.expected(i, capi.FMT_S16LE))


# ---- the far variant (tests/test_gpu_far_offsets.py): offsets past 32 bits ----------------------------------------------------------------

def _straddles(runs, boundary):
    return [r for r in runs if r[0] < boundary < r[1]]


@pytest.mark.parametrize("level", LEVELS)
def test_far_builder_properties(level):
    """what keeps the GPU tests over far_contract(level) from passing vacuously: the descriptors are valid and the near contract's, on
    every residue; nothing overlaps; every boundary lies inside a slot, a copy or a header run, with data on both sides; the alias rule"""
    ct, fc = AC.contract(level), AC.far_contract(level)
    cols, T = fc.cols, fc.T
    E30, E31, E32, H29 = AC.E30, AC.E31, AC.E32, AC.H29
    # the near contract's descriptors, every one once, reading the same copy of the same source
    assert sorted(fc.near_index) == list(range(len(ct.descs)))
    for j, i in enumerate(fc.near_index):
        d, n = fc.descs[j], ct.descs[i]
        assert (d.n_emit, d.level, d.rows, d.nrows, d.row_begin) == (n.n_emit, n.level, n.rows, n.nrows, n.row_begin)
        assert (fc.desc_source[j], fc.desc_copy[j]) == (ct.desc_source[i], ct.desc_copy[i])
        assert d.idx_off % 64 == n.idx_off % 64 and d.hdr_off % 2 == n.hdr_off % 2 and d.hdr_off > 0 and AC.valid_desc(d)
        assert d.idx_off == fc.idx_off[(fc.desc_source[j], fc.desc_copy[j])] and d.hdr_off == fc.hdr_off[(fc.desc_source[j], fc.desc_copy[j])]
        assert d.hdr_off + fc.sources[fc.desc_source[j]].st.info.blocks <= 1 << 32
    assert {d.idx_off % 64 for d in fc.descs} == {d.pcm_off % 64 for d in fc.descs} == set(range(0, 64, 8))
    assert {d.n_emit % 8 for d in fc.descs} == set(range(8))
    if fc.patches is not None:
        assert {p.stream for p in fc.patches} == {j for j, k in enumerate(fc.desc_source) if fc.sources[k].name == "C"}
    # runs: consecutive, each with descriptors from row 0 and windows, of every source and copy
    assert fc.desc_run == sorted(fc.desc_run) and set(fc.desc_run) == set(range(AC.FAR_RUNS))
    for r in range(AC.FAR_RUNS):
        js = [j for j, x in enumerate(fc.desc_run) if x == r]
        assert {fc.descs[j].row_begin == 0 for j in js} == {True, False}
        assert {fc.desc_source[j] for j in js} == set(range(len(fc.sources))) and {fc.desc_copy[j] for j in js} == set(range(AC.COPIES))
    # PCM slots: ascending, 8 guard words and more apart, run 0 near; each boundary strictly inside a slot of at least a tile and within 64
    # elements in front of the next slot's start
    starts = [s[0] for s in fc.slots]
    assert all(a[1] + 8 <= b[0] for a, b in zip(fc.slots, fc.slots[1:])) and fc.pcm_words == fc.slots[-1][1] + 64 > E32
    assert all(s[1] < E30 // 2 for s, r in zip(fc.slots, fc.desc_run) if r == 0)
    for r, b in ((1, E30), (2, E31), (3, E32)):
        (s,) = _straddles(fc.slots, b)
        assert s[3] == fc.straddler[r] and fc.desc_run[s[3]] == r and s[1] - s[0] >= T * cols
        assert 0 < min(x for x in starts if x > b) - b <= 64
        assert min(x for x in starts if x > b) == fc.slots[s[3] + 1][0] and fc.desc_run[s[3] + 1] == r
    fc.check_pcm_aliases()
    # index arena: the copies with 8 words of poison around them, apart; copy 0 where the near contract has it; a copy 1 astride E31, a copy
    # 2 astride E32; every source with staged rows on both sides of both
    runs = sorted(fc._idx_runs)
    assert all(a[1] + 16 <= b[0] for a, b in zip(runs, runs[1:])) and runs[0][0] >= 8 and fc.idx_words >= runs[-1][1] + 64
    for k, s in enumerate(fc.sources):
        assert fc.idx_off[(k, 0)] == s.idx_off[0]
        mine = [r for r in runs if r[2] == k]
        for b in (E31, E32):
            assert any(r[0] < b for r in mine) and any(r[1] > b for r in mine)
    assert [r[3][1] for r in _straddles(runs, E31)] == [1] and [r[3][1] for r in _straddles(runs, E32)] == [2]
    for o, a in fc.idx_pieces:
        assert (a[:8] == AC.IDX_POISON).all() and (a[-8:] == AC.IDX_POISON).all()
    assert all(a[0] + a[1].size <= b[0] for a, b in zip(fc.idx_pieces, fc.idx_pieces[1:]))
    AC.check_aliases(fc._idx_runs, (E31, E32), {k: s.st.idx[:s.nrows * cols] for k, s in enumerate(fc.sources)}, fc.idx_displaced)
    assert set(fc.idx_displaced) <= {(1, 2)}        # (only B's copy astride E32, whose rows in front of E32 alias to B's in front of E31)
    # header arena: copies 0 and 1 near, a run astride entry 2^29, runs on both sides, a poison header in front of each
    hruns = sorted(fc._hdr_runs)
    assert all(a[1] + 1 <= b[0] for a, b in zip(hruns, hruns[1:])) and len(_straddles(hruns, H29)) == 1
    for k, s in enumerate(fc.sources):
        assert [fc.hdr_off[(k, c)] for c in (0, 1)] == s.hdr_off[:2] and all(fc.hdr_off[(k, c)] + s.st.info.blocks > H29 - 64 for c in (2, 3))
    assert any(r[0] >= H29 for r in hruns)          # (in front of entry 2^29: the straddling run's first headers, and copies 0 and 1)
    for o, a in fc.hdr_pieces:
        assert tuple(a[0]) == AC.HDR_POISON
    AC.check_aliases(fc._hdr_runs, (H29,), {k: s.st.hdr[:s.st.info.blocks] for k, s in enumerate(fc.sources)}, fc.hdr_displaced)
    assert not fc.hdr_displaced


def _local(pieces, off, length, lead):
    """the piece that holds [off, off + length) and where `off` lies in it"""
    for o, a in pieces:
        if o <= off and off + length <= o + len(a):
            assert off - o >= lead
            return a, off - o
    raise AssertionError("no piece holds %d" % off)


@pytest.mark.parametrize("fmt", [capi.FMT_S16LE, AC.F32])
@pytest.mark.parametrize("level", LEVELS)
def test_host_synth_on_far_pieces(level, fmt):
    """the far contract's pieces and descriptors belong together: acmhip_host_synth / _f32 of every far descriptor, handed the pieces that
    hold its copy and its header run with the offsets counted from the pieces' own starts (NOT the far offsets: the host synthesis never
    sees an offset past 32 bits here, and no pointer is formed outside an allocation) and a slot of its own with the slot's residue
    modulo 64, gives the oracle's slice and leaves the guard words around the slot alone"""
    import ctypes as C
    fc, L = AC.far_contract(level), capi.lib()
    poison = AC.POISON32 if fmt == AC.F32 else AC.POISON16
    for j, d in enumerate(fc.descs):
        s = fc.sources[fc.desc_source[j]]
        idx, io = _local(fc.idx_pieces, d.idx_off, s.nrows * fc.cols, 8)
        hdr, ho = _local(fc.hdr_pieces, d.hdr_off, s.st.info.blocks, 1)
        assert io % 8 == 0
        po = 64 + d.pcm_off % 64
        out = np.full(po + d.n_emit + 64, poison, dtype=np.uint32 if fmt == AC.F32 else np.uint16)
        loc = capi.StreamDesc(idx_off=io, hdr_off=ho, pcm_off=po, n_emit=d.n_emit, level=d.level, rows=d.rows, nrows=d.nrows, row_begin=d.row_begin)
        arr = (capi.Patch * len(s.patches))(*s.patches) if s.patches else None
        hdr = np.ascontiguousarray(hdr)
        if fmt == AC.F32:
            rc = L.acmhip_host_synth_f32(C.byref(loc), idx.ctypes.data, hdr.ctypes.data, arr, len(s.patches), out.ctypes.data)
        else:
            rc = L.acmhip_host_synth(C.byref(loc), idx.ctypes.data, hdr.ctypes.data, arr, len(s.patches), fmt, out.ctypes.data)
        assert rc == 0, fc.describe(j)
        assert np.array_equal(out[po:po + d.n_emit], fc.expected(j, fmt)), fc.describe(j)
        assert (out[:po] == poison).all() and (out[po + d.n_emit:] == poison).all(), fc.describe(j)


def test_far_words_are_described():
    """describe_word: a dirty word names the descriptor in front of it and the distance behind its n_emit, like Contract.check, and the
    slot or boundary it is an alias of"""
    fc = AC.far_contract(4)
    j = fc.straddler[3]
    lo, hi = fc.slots[j][:2]
    assert ("word %d lies 2 words behind the n_emit of desc %d " % (hi + 2, j)) in fc.describe_word(hi + 2)
    assert (", %d words in front of desc %d" % (fc.slots[j + 1][0] - hi - 2, j + 1)) in fc.describe_word(hi + 2)
    assert ("is sample 3 of desc %d " % j) in fc.describe_word(lo + 3)
    assert "in front of the first slot" in fc.describe_word(5) and "5 words behind the alias of boundary E32" in fc.describe_word(5)
    assert ("the alias modulo E31 of sample 7 of desc %d" % j) in fc.describe_word(lo + 7 - AC.E31)
    assert ("the alias modulo E30 of sample 7 of desc %d" % j) in fc.describe_word(lo + 7 - 3 * AC.E30)
    assert sum(b - a for a, b in fc.gaps()) + sum(d.n_emit for d in fc.descs) == fc.pcm_words


@pytest.mark.parametrize("level,form", [(lv, "byteplane") for lv in range(7, 15)] + [(lv, "packed") for lv in range(6, 10)])
def test_far_forms(level, form):
    """the relocated second forms: copies 0 and 1 near, the blob regions and table runs of copies 2 and 3 on both sides of byte 2^32 with
    one astride it; each run's entries, their blob offsets rebased, name the run's own region - and decode back to the source's staged
    indices there; the alias rule (FarForm, lay_far assert it; here: nothing overlaps, nothing is displaced)"""
    fc, ff = AC.far_contract(level), AC.far_form(level, form)
    L, B32 = capi.lib(), AC.B32
    assert not ff.blob_displaced and not ff.table_displaced
    for pieces, boundary in ((ff.blob_pieces, B32), (ff.table_pieces, ff.table_boundary)):
        runs = [(o, o + len(a)) for o, a in pieces]
        assert all(a[1] <= b[0] for a, b in zip(runs, runs[1:]))
        assert len(_straddles(runs, boundary)) == 1 and any(r[0] >= boundary for r in runs) and sum(r[1] < boundary // 2 for r in runs) == 2 * len(fc.sources)
    assert ff.table_boundary * ff.unit == B32 and ff.table_bytes > B32 and ff.blob_bytes > B32
    offs = sorted(p.chunk_off for p in ff.streams)
    assert offs[0] < ff.table_boundary < offs[-1] < 1 << 32
    tr = L.acmhip_mform_tile_rows(level) if form == "byteplane" else L.acmhip_packed_tile_rows(level)
    # the region and the table run astride byte 2^32 are read: a descriptor from row 0 with a whole lean tile has them as its form
    t2 = L.acmk_tile2_rows(level)
    lean = {(fc.desc_source[j], fc.desc_copy[j]) for j, d in enumerate(fc.descs) if ff.streams[j].ntiles and d.row_begin == 0 and d.n_emit >> level >= t2}
    assert {q for q, o in ff.blob_off.items() if o < B32 < o + dict(ff.blob_pieces)[o].size} <= lean
    assert {q for q, o in ff.table_off.items() if o < ff.table_boundary < o + ff.count[q]} <= lean
    assert any(ff.blob_off[q] > B32 for q in lean) and any(ff.table_off[q] > ff.table_boundary for q in lean)
    for (k, c), at in ff.table_off.items():
        entries = dict(ff.table_pieces)[at]
        region = dict(ff.blob_pieces)[ff.blob_off[(k, c)]]
        lo, hi = ff.blob_off[(k, c)], ff.blob_off[(k, c)] + region.size
        rows = ff.ntiles[(k, c)] * tr
        want = fc.sources[k].st.idx[:rows * fc.cols]
        if form == "byteplane":
            assert all(lo <= int(e >> 2) * 64 < hi for e in entries)
            local = entries - np.uint32((lo // 64) << 2)
            assert np.array_equal(capi.mform_unrows(level, region, local, rows), want), (k, c)
        else:
            used = entries[entries["kind"] != 0]
            assert ((used["blob_off16"].astype(np.int64) * 16 >= lo) & (used["blob_off16"].astype(np.int64) * 16 < hi)).all()
            local = entries.copy()
            local["blob_off16"][local["kind"] != 0] -= lo // 16
            slots = L.acmhip_packed_slots(level)
            got = np.concatenate([capi.unpack_tile(level, local, region, t * slots).reshape(-1) for t in range(ff.ntiles[(k, c)])])
            assert np.array_equal(got, want), (k, c)
    for j, p in enumerate(ff.streams):
        assert (p.ntiles == 0) == bool(fc.sources[fc.desc_source[j]].patches) and p.chunk_off == ff.table_off[(fc.desc_source[j], fc.desc_copy[j])]
