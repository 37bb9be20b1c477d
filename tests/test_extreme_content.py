"""The crafted streams of tests/extreme_content.py, without a GPU: the writer writes what it was given, the aligned streams reach the
bound the coefficient tables allow (a numpy model of the first stages, one operand plane at a time - DESIGN.md 2.1), every stream
travels in the width class it was made for, the planner sends them down the paths they were made for, and the product's host
synthesis decodes every one of them like the oracle.  tests/test_gpu_extreme_content.py runs the same streams through the kernels."""
import collections

import numpy as np
import pytest

import extreme_content as X
import test_plan_cut as PC
from helpers import crafted_stream, fmt_args, oracle_pcm
from libacm_amd import capi
from test_host_synth import host_synth

ALL_LEVELS = list(range(16))
FORM_LEVELS = list(range(7, 15))


def whole_desc(s):
    info = s.info
    return capi.StreamDesc(idx_off=0, hdr_off=0, pcm_off=0, n_emit=info.blocks * info.rows << info.level, level=info.level, rows=info.rows,
                           nrows=info.blocks * info.rows, row_begin=0)


# ---------------------------------------------------------------------------------------------------------------- the writer

def test_writer_bit_order_and_checks():
    """one small block by hand: header bytes, the 5-bit code and the fillers LSB first; the range checks refuse what would need an H1 patch"""
    idx = np.array([[-4, 3], [0, -1]])
    f = crafted_stream(1, 2, [(2, 0x1234, 3, idx)], channels=1, cut=1)
    assert f[:4] == bytes([0x97, 0x28, 0x03, 0x01]) and f[4:8] == bytes([3, 0, 0, 0]) and f[8:12] == bytes([1, 0, 0x22, 0x56])
    s = capi.stage_file(f)
    assert np.array_equal(s.idx, idx.reshape(-1)) and s.hdr.tolist() == [[0x1234, 2]] and s.info.total_values == 3
    with pytest.raises(AssertionError):
        crafted_stream(1, 2, [(2, 1, 3, idx + 1)])            # 4 is outside a 3-bit filler
    with pytest.raises(AssertionError):
        crafted_stream(1, 2, [(1, 1, 3, idx)])                # code > pwr + 1: indices outside the block's table
    with pytest.raises(AssertionError):
        crafted_stream(1, 2, [(2, 1, 3, idx[:1])])


@pytest.mark.parametrize("level", ALL_LEVELS)
def test_writer_round_trip(level):
    """the host stager reads back the indices and headers that were put in, without patches; the oracle decodes the file with status 0"""
    streams = X.level_streams(level)
    want = X.level_oracle(level)
    assert len(streams) >= 30
    for s, (pcm, status) in zip(streams, want):
        st = capi.stage_file(s.data)
        bl = st.block_len                     # (the stager stops behind the block that holds the last of total_values)
        assert st.idx.size == (s.idx.size - 3 + bl - 1) // bl * bl and st.info.end_status == 0, s.name
        assert np.array_equal(st.idx, s.idx.reshape(-1)[:st.idx.size]), s.name
        assert np.array_equal(st.hdr, s.hdr[:st.info.blocks]), s.name
        assert st.patches is None and st.info.npatches == 0, s.name
        assert status == 0 and pcm.size == s.idx.size - 3, s.name


@pytest.mark.parametrize("level", list(range(5, 16)))
def test_block_structure(level):
    """every family x class at every block height; header values from the list - a stream of tall blocks begins with one the chunk
    kernel's fast path takes -, pwr the smallest that admits the block's indices"""
    seen = collections.defaultdict(set)
    vals = set(X.header_values(level))
    for s in X.level_streams(level):
        seen[(s.family, s.cls.name if s.cls else None)].add(s.height)
        h = {"1": 1, "3": 3, "tall": 2 * X.plan_rows(level)}[s.height]
        assert s.idx.shape[0] >= 4 * X.plan_rows(level) + 1 and s.idx.shape[0] % h == 0
        assert set(s.hdr[:, 0].tolist()) <= vals
        assert s.height != "tall" or (len(s.hdr) == 3 and X.fast_value(level, int(s.hdr[0, 0]))), s.name
        for b, (val, pwr) in enumerate(s.hdr.tolist()):
            blk = s.idx[b * h:(b + 1) * h].astype(np.int64)
            assert -(1 << pwr) <= blk.min() and blk.max() < 1 << pwr
            assert pwr == 2 or blk.min() < -(1 << pwr >> 1) or blk.max() >= 1 << pwr >> 1
    want = {(f, c.name) for f in X.level_families(level) if f != "border" for c in X.level_classes(level)} | {("border", None)}
    assert set(seen) == want and all(v == set(X.HEIGHTS) for v in seen.values()), seen
    assert {65535, 0, 1} <= {int(v) for s in X.level_streams(level) for v in s.hdr[:, 0]}


# ---------------------------------------------------------------------------------------------------------------- reach

def test_response_is_the_toeplitz_operator_of_the_table_generator():
    """the impulse responses derived here and by tools/gen_mfma_tables.py (two restatements of the stage formula) agree"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("gen_mfma_tables", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "gen_mfma_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for G in (3, 6):
        (t0, t1, t2), _ = gen.toeplitz(G)
        assert np.array_equal(X.response(G), np.concatenate([t2, t1, t0], axis=1))
    R = X.response(6)
    assert np.abs(R).max() <= 64 and np.abs(R).sum(axis=1).max() == 1822
    assert (R.sum(axis=1).min(), R.sum(axis=1).max()) == (-608, 576)
    assert 128 * 1822 < 1 << 18


@pytest.mark.parametrize("level", FORM_LEVELS)
def test_aligned_streams_reach_the_bound(level):
    """The first G stages over each operand plane of every aligned stream, in int64: over the streams of a class the largest and the
    smallest plane sum ARE what the coefficients allow for that plane's operand range - sum of c * max over c > 0 plus c * min over c < 0,
    and its mirror - at some output q.  (Level 9, 8-bit operands: +232 353 / -232 257 of the 233 216 that 1822 * 128 would allow.)
    And they are reached where the chunk kernel's fast path computes them: in the streams of tall blocks of every class but the
    whole-range one, in a row with both rows of its history in its own block, under a header value that path takes (X.fast_value) -
    whatever order the streams are made in."""
    G, cols = X.stages(level), 1 << level
    h = 2 * X.plan_rows(level)
    got = collections.defaultdict(lambda: [0, 0])
    fast = collections.defaultdict(lambda: [0, 0])
    for s in X.level_streams(level):
        if s.family != "aligned":
            continue
        for name, plane in zip(("lo", "hi"), X.planes(s.cls, s.idx)):
            if plane is not None:
                y = X.first_stages(plane, cols, G)
                g = got[(s.cls.name, name)]
                g[0], g[1] = max(g[0], int(y.max())), min(g[1], int(y.min()))
                if s.height == "tall":
                    for b in np.nonzero([X.fast_value(level, int(v)) for v in s.hdr[:, 0]])[0]:
                        yb = y.reshape(-1, cols)[b * h + 2:(b + 1) * h]
                        g = fast[(s.cls.name, name)]
                        g[0], g[1] = max(g[0], int(yb.max())), min(g[1], int(yb.min()))
        if "0" not in s.meta["signs"] and (s.cls.name != "wr" or s.meta["signs"] in ("++", "--")):
            assert s.meta["touched"] == 0, s.name          # in their class by themselves: no index was bent to get there
    assert set(got) == {(c.name, p) for c in X.level_classes(level) for p in (("lo", "hi") if c.hi else ("lo",))}
    for c in X.level_classes(level):
        for name, rng_ in (("lo", c.lo), ("hi", c.hi)):
            if rng_ is not None:
                hi, lo = X.bounds(G, rng_)
                print("level %d class %s plane %s: reached %+d / %+d, bound %+d / %+d" % (level, c.name, name, *got[(c.name, name)], hi.max(), lo.min()))
                assert got[(c.name, name)] == [int(hi.max()), int(lo.min())], (c.name, name)
                if c.name != "wr":
                    assert fast[(c.name, name)] == [int(hi.max()), int(lo.min())], (c.name, name, fast[(c.name, name)])
                assert max(hi.max(), -lo.min()) < 1 << 18
    if G == 6:
        assert got[("8", "lo")][0] > 1 << 17 and got[("8", "lo")][1] < -(1 << 17)          # bits 17 and 18 of a plane sum are in play


# ---------------------------------------------------------------------------------------------------------------- class

@pytest.mark.parametrize("level", FORM_LEVELS)
def test_streams_travel_in_their_class(level):
    """every pair of a stream made for one class is stored in it (acmhip_mform_rows), every pair of every stream in the class
    tests/test_byteplane_form.py expects for its indices, each border pair in the class on ITS side of the border"""
    tr = capi.lib().acmhip_mform_tile_rows(level)
    classes_seen = set()
    for s in X.level_streams(level):
        st = capi.stage_file(s.data)
        mf = capi.mform_streams(st.idx, [whole_desc(st)])
        npairs = mf.streams[0].ntiles * tr // 2
        assert npairs >= 2 * X.plan_rows(level)
        cls = mf.pairs[1:1 + npairs] & 3
        rows = s.idx[:2 * npairs].reshape(npairs, -1).astype(np.int64)
        want = [X.expected_class(level, int(lo), int(hi)) for lo, hi in zip(rows.min(axis=1), rows.max(axis=1))]
        assert cls.tolist() == want, s.name
        if s.family == "border":
            assert cls.tolist() == s.meta["pair_class"][:npairs], s.name
            classes_seen |= set(cls.tolist())
        elif s.family == "impulse":
            p = s.meta["row"] // 2
            assert cls[p] == s.cls.code and (np.delete(cls, p) == (1 if level == 7 else 2)).all(), s.name
        else:
            assert (cls == s.cls.code).all(), (s.name, cls)
    assert classes_seen == {c.code for c in X.level_classes(level)}


# ---------------------------------------------------------------------------------------------------------------- path

@pytest.mark.parametrize("level", [8, 9, 10, 11, 12])
def test_tall_blocks_make_oneblock_chunks(level):
    """the planner's chunk records (acmk_plan_cut_visit, as tests/test_plan_cut.py cuts them): a stream of blocks two tiles high has
    chunks whose rows in reach lie in one block (ACM_TILE_ONEBLOCK: with one width throughout, the chunk kernel's fast path at 8, 12
    and 16 bits); a stream of one-row blocks has none behind its first chunk (a chunk of ONE row at row 0 - levels 11 and 12 - has no row
    in front of it, and so one block in reach whatever the block height)"""
    L = PC._lib()
    for height in ("tall", "1"):
        streams = [s for s in X.level_streams(level) if s.height == height]
        assert {s.cls.name for s in streams if s.cls} == {c.name for c in X.level_classes(level)}
        ar = capi.Arena([capi.stage_file(s.data) for s in streams])
        mf = capi.mform_streams(ar.idx, ar.descs)
        res = PC.run_case(L, PC.Case("crafted", 256, capi.PLAN_LEAN_ALWAYS, ar.descs, mf.streams))
        assert res["rc"] == 0, res["err"]
        rec = PC.decode(res)[("tiles2m", level)]
        live = rec[(rec["flags"] & PC.TILE_DISCARD) == 0]
        owner = np.searchsorted([d.pcm_off for d in ar.descs], live["pcm_off"], side="right") - 1
        one = np.bincount(owner[(live["flags"] & PC.TILE_ONEBLOCK) != 0], minlength=len(streams))
        one_behind = np.bincount(owner[(live["flags"] & (PC.TILE_ONEBLOCK | PC.TILE_FRESH)) == PC.TILE_ONEBLOCK], minlength=len(streams))
        assert np.bincount(owner, minlength=len(streams)).min() > 0
        if height == "tall":
            assert one.min() > 0, [s.name for s, n in zip(streams, one) if n == 0]
        else:
            assert one_behind.max() == 0 and one.max() <= (capi.lib().acmhip_mform_tile_rows(level) == 1)


# ---------------------------------------------------------------------------------------------------------------- host synthesis

@pytest.mark.parametrize("level,fmt", [(lv, capi.FMT_S16LE) for lv in ALL_LEVELS] + [(9, f) for f in (capi.FMT_S16BE, capi.FMT_U16LE, capi.FMT_U16BE)])
def test_host_synthesis(level, fmt):
    """acmhip_host_synth over every crafted stream: bit-exact PCM (all four formats at level 9)"""
    be, sg = fmt_args(fmt)
    for s, (pcm, _) in zip(X.level_streams(level), X.level_oracle(level)):
        want = pcm if fmt == capi.FMT_S16LE else oracle_pcm(s.data, 0, be, sg)[0]
        got = host_synth(capi.stage_file(s.data), fmt=fmt)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "%s: %d samples differ, first at %d" % (s.name, bad.size, bad[0])
