"""The arena contract of include/acm_hip.h without a GPU: the builder of tests/arena_contract.py has the properties the GPU test
(tests/test_gpu_arena_contract.py) relies on, and the library's host synthesis keeps the contract on those arenas.

acmhip_host_synth / acmhip_host_synth_f32 take the same descriptor as a plan; the other host tests call them with idx_off = hdr_off =
pcm_off = 0.  Here every descriptor of every level runs on the contract arena with the arena's own offsets (8-word residues, headers
behind poison headers, ragged n_emit, windows), in the four 16-bit formats and in float32: every slot is the oracle's slice and every
word outside [pcm_off, pcm_off + n_emit) keeps its poison.  That the expectations come out right here is also what makes a failure of
the GPU test the kernels' and not the builder's."""
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
