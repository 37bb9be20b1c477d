"""Direct oracle-vs-reference sweeps: the oracle against what the compiled reference answered for the same streams.  The
reference's answers (status and PCM digest per stream, digests of its juggle_block) are replayed from tests/golden/ref_answers.json,
recorded from oracle/_ref by tests/golden/make_golden_ref_answers.py; the committed golden vectors (test_oracle_golden.py) pin the
rest."""
import numpy as np
import pytest

import oracle_api as O
from helpers import RefAnswers, make_stream, sha


def ref_decode(data, force_chans, be, sgned):
    r = O.LibacmStream(O.ref_lib(), data, force_chans)
    if r.err < 0:
        return [r.err]
    pcm, st = r.decode_all(8192, be, sgned)
    r.close()
    return [0, st, sha(pcm)]


def both(ans, data, **kw):
    fc, be, sgned = kw.get("force_chans", 0), kw.get("be", 0), kw.get("sgned", 1)
    want = ans.ask(lambda: ref_decode(data, fc, be, sgned))
    if want[0] < 0:
        o = O.Oracle(data, fc)
        assert o.err == want[0]
        return
    po, so = O.Oracle.decode_all(data, fc, be=be, sgned=sgned)
    assert [so, sha(po.tobytes())] == want[1:]


@pytest.mark.parametrize("level", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15])
def test_random_matrix(level):
    """levels 13-15 have kernels of their own (prefix sweep + plane kernel, acm_tile2 with the shared first pass): the oracle those are
    held to is held to the reference here, at block heights 1, 2 and 5"""
    ans = RefAnswers("test_oracle_vs_ref::test_random_matrix[%d]" % level)
    for rows in (1, 2, 3, 16, 17, 64) if level <= 12 else (1, 2, 5):
        if level >= 11 and rows > 17:
            continue
        for ch in (1, 2):
            for mix in (0, 1):
                both(ans, make_stream(level * 977 + rows * 13 + ch + mix * 7, level, rows, 4, channels=ch, cut=3, mix=mix))
    ans.done()


@pytest.mark.parametrize("shape", [(0, 4095, 3), (3, 4095, 2), (5, 4095, 3), (9, 4095, 2), (11, 700, 2), (13, 64, 2), (12, 4095, 1)])
def test_tall_blocks(shape):
    """(level, rows, blocks): the 12-bit row count at its end, and blocks taller than 64 rows at the upper levels"""
    level, rows, nb = shape
    ans = RefAnswers("test_oracle_vs_ref::test_tall_blocks[%s]" % (shape,))
    both(ans, make_stream(level * 31 + rows, level, rows, nb, channels=1 + (level & 1), cut=3, mix=(rows >> 1) & 1))
    ans.done()


def test_extreme_values_and_stale_table():
    ans = RefAnswers("test_oracle_vs_ref::test_extreme_values_and_stale_table")
    for seed in range(20):
        both(ans, make_stream(3000 + seed, 5, 7, 8, mix=1, allow_out_of_range=1, prime_table=1, pwr_min=0, pwr_max=15,
                              val_min=0, val_max=65535))
    ans.done()
    # the same material at the other ends of the level range (a key of its own: the answers above stay as they were recorded)
    ans = RefAnswers("test_oracle_vs_ref::test_extreme_values_and_stale_table[levels]")
    for level in (0, 2, 9, 12, 13, 15):
        for seed in range(6):
            both(ans, make_stream(3100 + 10 * level + seed, level, 7 if level < 12 else 3, 8 if level < 12 else 4, mix=1, allow_out_of_range=1,
                                  prime_table=1, pwr_min=0, pwr_max=15, val_min=0, val_max=65535))
    ans.done()


def test_random_truncations():
    rng = np.random.default_rng(5)
    f = make_stream(99, 7, 16, 6)
    ans = RefAnswers("test_oracle_vs_ref::test_random_truncations")
    for n in rng.integers(0, len(f), size=200):
        both(ans, f[:int(n)])
    ans.done()


def test_bit_flips():
    rng = np.random.default_rng(6)
    # block 0 primes the whole amplitude table (pwr 15), flips stay behind it: a flipped pwr/code may then
    # index "stale" entries, but never uninitialised heap (which the reference would read as garbage)
    f = bytearray(make_stream(98, 6, 8, 6, prime_table=1))
    ans = RefAnswers("test_oracle_vs_ref::test_bit_flips")
    for _ in range(300):
        g = bytearray(f)
        pos = int(rng.integers(len(g) // 3, len(g)))
        g[pos] ^= 1 << int(rng.integers(0, 8))
        both(ans, bytes(g))
    ans.done()


def test_cascade_formulation_equals_reference_juggle():
    """juggle_block == `level` strided 3-tap FIR stages over the flat sample index,
    history = zeros, chunking irrelevant.  This is the formulation the HIP kernels implement."""
    rng = np.random.default_rng(7)
    shapes = [(level, rows) for level in (1, 2, 3, 5, 7, 9, 10) for rows in (1, 3, 16, 17)]
    # (a key of their own: the answers of the shapes above stay as they were recorded)
    more = [(level, rows) for level in (4, 6, 8, 11, 12) for rows in (1, 3, 17)] + [(level, rows) for level in (13, 14, 15) for rows in (1, 3)]
    for key, todo in (("", shapes), ("[more]", more)):
        ans = RefAnswers("test_oracle_vs_ref::test_cascade_formulation_equals_reference_juggle" + key)
        for level, rows in todo:
            cols = 1 << level
            nb = 4
            x = rng.integers(-2 ** 31, 2 ** 31 - 1, size=nb * rows * cols, dtype=np.int64).astype(np.int32)

            def ref_juggle():
                P = O.refprobe_lib()
                wrap = np.zeros(max(1, 2 * cols - 2), dtype=np.int32)
                ref = x.copy()
                for b in range(nb):
                    blk = np.ascontiguousarray(ref[b * rows * cols:(b + 1) * rows * cols])
                    P.refprobe_juggle_block(level, rows, blk.ctypes.data, wrap.ctypes.data)
                    ref[b * rows * cols:(b + 1) * rows * cols] = blk
                return sha(ref.tobytes())
            want = ans.ask(ref_juggle)
            y = x.astype(np.uint32)
            m = np.arange(y.size)
            for k in range(level):
                s = cols >> (k + 1)
                x1 = np.concatenate([np.zeros(s, np.uint32), y[:-s]]) if s < y.size else np.zeros_like(y)
                x2 = np.concatenate([np.zeros(2 * s, np.uint32), y[:-2 * s]]) if 2 * s < y.size else np.zeros_like(y)
                odd = ((m // s) & 1).astype(bool)
                y = np.where(odd, 2 * x1 - (x2 + y), 2 * x1 + (x2 + y)).astype(np.uint32)
                if k == 0:
                    y = (y + (m % (cols // 2) == 0 if cols >= 2 else 1)).astype(np.uint32)
            assert sha(np.ascontiguousarray(y.view(np.int32)).tobytes()) == want, (level, rows)
        ans.done()
