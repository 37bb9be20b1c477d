"""Streams whose INDICES are chosen (helpers.crafted_stream), so that the matrix first pass of acm_chunk / acm_tile2 meets the corners of
its arithmetic: plane sums at the bound the coefficient tables allow, every width class at both of its ends, the
borders between the classes, single extreme indices in an otherwise silent stream.  Pure numpy, no device.

The first G stages of the cascade over one residue class of the columns - columns c + q * cols / 2^G - are
out[r] = T0 x[r] + T1 x[r-1] + T2 x[r-2]; response(G)[q] is row q of [T2 | T1 | T0], derived here by pushing impulses through the
stage formula (never read from the library's tables).  G is what the level's matrix build runs: 3 at level 7, 6 at levels 8-14; the
levels without a matrix build take the same content with G = 3 below level 8 and 6 above (it is just loud material there).

Width classes, as the byte-plane form stores them (include/acm_hip.h; `split` says how an index becomes the matrix operands):
  level 7      "4" [-8, 7] and "8" [-128, 127] one plane; "16" idx = 256 hi + (lo + 128), both planes in [-128, 127]
  levels 8-14  "8"; "12" (levels 8-12) idx = 256 hi + lo, lo a signed byte, hi a signed nibble: [-2176, 1919]; "16" the same with a
               signed high byte, ends at 32639; "wr" (whole range, a pair with an index >= 32640) idx = 256 hi + (lo + 128)
"""
import functools
from collections import namedtuple

import numpy as np

from helpers import crafted_stream, oracle_pcm, plan_rows

Cls = namedtuple("Cls", "name code split lo hi idx")              # code: pair-table code; lo / hi: operand range per plane; idx: index range
Stream = namedtuple("Stream", "name family cls height data idx hdr meta")

BYTE, NIB = (-128, 127), (-8, 7)
CLS4 = Cls("4", 1, None, NIB, None, NIB)
CLS8 = Cls("8", 2, None, BYTE, None, BYTE)
CLS12 = Cls("12", 1, "s", BYTE, NIB, (-2176, 1919))
CLS16 = Cls("16", 3, "s", BYTE, BYTE, (-32768, 32639))
CLS16U = Cls("16", 3, "u", BYTE, BYTE, (-32768, 32767))           # level 7: the low byte unsigned, stored minus 128
CLSWR = Cls("wr", 0, "u", BYTE, BYTE, (-32768, 32767))
HEIGHTS = ("1", "3", "tall")
FAMILIES = ("aligned", "constant", "checker", "border", "impulse")


def stages(level):
    return 3 if level < 8 else 6


def level_classes(level):
    if level == 7:
        return [CLS4, CLS8, CLS16U]
    if 8 <= level <= 12:
        return [CLS8, CLS12, CLS16, CLSWR]
    if level in (13, 14):
        return [CLS8, CLS16, CLSWR]
    return [CLS8, CLSWR]                    # no byte-plane form: quiet and loud content


def level_families(level):
    return FAMILIES if level >= 5 else ("constant", "checker", "impulse")       # levels 0-4: no matrix pass, no width classes


def header_values(level):
    """block header values in turn; from level 10 on the kernels pre-scale val, and `border` is where it leaves 16 bits"""
    border = 65536 >> (16 - level)
    return [65535, 0, 65535, 1, 255] + ([border - 1, border] if level >= 10 else [])


# ---------------------------------------------------------------------------------------------------------------- the model

def first_stages(x, cols, G):
    """stages 0 .. G-1 of DESIGN.md 1 over the flat sample index, int64, without the "+1" (a model of ONE operand plane)"""
    v = np.asarray(x, dtype=np.int64).reshape(-1)
    m = np.arange(v.size)
    for k in range(G):
        s = cols >> (k + 1)
        x1, x2 = np.zeros_like(v), np.zeros_like(v)
        x1[s:] = v[:max(v.size - s, 0)]
        x2[2 * s:] = v[:max(v.size - 2 * s, 0)]
        v = 2 * x1 + np.where(m & s, -1, 1) * (x2 + v)
    return v


@functools.lru_cache(None)
def response(G):
    """[T2 | T1 | T0] as one (2^G, 3 * 2^G) matrix: row q = the coefficients of output q of a row over the class's inputs of the rows
    r-2, r-1, r (a class on its own is a stream of 2^G columns)"""
    U = 1 << G
    R = np.zeros((U, 3 * U), dtype=np.int64)
    for k in range(U):
        e = np.zeros(4 * U, dtype=np.int64)
        e[k] = 1
        y = first_stages(e, U, G)
        assert not y[3 * U:].any()          # the reach of G stages, 2 (2^G - 1) positions, stays inside two rows
        for j in range(3):
            R[:, (2 - j) * U + k] = y[j * U:(j + 1) * U]
    return R


def bounds(G, rng_):
    """(largest, smallest) sum the coefficients allow with operands in [rng_[0], rng_[1]], per output q"""
    R = response(G)
    pos, neg = np.maximum(R, 0).sum(axis=1), np.minimum(R, 0).sum(axis=1)
    return pos * rng_[1] + neg * rng_[0], pos * rng_[0] + neg * rng_[1]


def bound_outputs(G):
    """the outputs q where the bound of a byte plane and of a nibble plane is largest / smallest (the first of them: the largest sum of |c|)"""
    return list(dict.fromkeys(int(f(b)) for rng_ in (BYTE, NIB) for f, b in zip((np.argmax, np.argmin), bounds(G, rng_))))


def aligned_outputs(G):
    """the outputs q the aligned streams aim at: bound_outputs, then the largest and the smallest signed row sum"""
    R = response(G)
    qs = bound_outputs(G) + [int(np.argmax(R.sum(axis=1))), int(np.argmin(R.sum(axis=1)))]
    assert np.abs(R[qs[0]]).sum() == np.abs(R).sum(axis=1).max()
    return list(dict.fromkeys(qs))


def planes(cls, idx):
    """the operands (lo, hi) the matrix pass sees for these indices in this class (hi None: one plane)"""
    x = np.asarray(idx, dtype=np.int64)
    if cls.split is None:
        return x, None
    if cls.split == "s":
        lo = ((x & 0xFF) ^ 0x80) - 0x80
        return lo, (x - lo) >> 8
    return (x & 0xFF) - 128, x >> 8


def compose(cls, lo, hi):
    if cls.split is None:
        return lo
    if cls.split == "s":
        return np.clip(256 * hi + lo, *cls.idx)         # (-128, -128) is below an int16: (-128, 0)
    return 256 * hi + lo + 128


def expected_class(level, lo, hi):
    """the pair-table code of a row pair whose indices span [lo, hi]: tests/test_byteplane_form.py test_round_trip"""
    if level == 7:
        return 1 if (lo >= -8 and hi <= 7) else 2 if (lo >= -128 and hi <= 127) else 3
    if lo >= -128 and hi <= 127:
        return 2
    if lo >= -2176 and hi <= 1919 and level <= 12:
        return 1
    return 0 if hi >= 32640 else 3


# ---------------------------------------------------------------------------------------------------------------- content

def _keep_class(level, cls, idx, weight=None):
    """a width class is a matter of the PAIR: the whole-range class needs one index >= 32640, a split class with a silent high plane
    one index that has a high part.  A pair that would travel in another class gets the class's largest index where it matters least
    (`weight`: per column, default column 0) in its first row; returns how many pairs were bent that way"""
    n = 0
    col = 0 if weight is None else int(np.argmin(weight))
    for p in range(0, idx.shape[0] - 1, 2):
        if expected_class(level, int(idx[p:p + 2].min()), int(idx[p:p + 2].max())) != cls.code:
            idx[p, col] = cls.idx[1]
            n += 1
    return n


def aligned(level, cls, q, s_lo, s_hi, nrows):
    """rows r = 0, 1, 2 (mod 3) carry sign(T2[q]), sign(T1[q]), sign(T0[q]): output q of every third row sums all 3 * 2^G terms of
    a plane with one sign.  s_lo / s_hi: "+" aligned, "-" anti-aligned, "0" that plane silent."""
    G, cols = stages(level), 1 << level
    U = 1 << G
    sign = np.where(response(G)[q] >= 0, 1, -1).reshape(3, U)

    def pick(s, rng_):
        if s == "0":
            return np.zeros_like(sign)
        if s == "+":
            return np.where(sign > 0, rng_[1], rng_[0])
        return np.where(sign > 0, rng_[0], rng_[1])
    pat = compose(cls, pick(s_lo, cls.lo), pick(s_hi, cls.hi) if cls.hi else None)
    idx = np.repeat(pat, cols // U, axis=1)[np.arange(nrows) % 3]
    touched = _keep_class(level, cls, idx, np.abs(response(G)[q]).reshape(3, U).min(axis=0).repeat(cols // U))
    return idx, {"q": q, "signs": s_lo + s_hi, "touched": touched}


def constant(level, cls, end, nrows):
    idx = np.full((nrows, 1 << level), cls.idx[end], dtype=np.int64)
    return idx, {"touched": _keep_class(level, cls, idx)}


def checker(level, cls, kind, nrows):
    """the class's two ends alternating: kind "col" / "row" by parity, k by bit log2(cols) - 1 - k of the column (stage k's sg pattern)"""
    cols = 1 << level
    r, c = np.meshgrid(np.arange(nrows), np.arange(cols), indexing="ij")
    up = (c & 1) if kind == "col" else (r & 1) if kind == "row" else (c >> (level - 1 - kind)) & 1
    idx = np.where(up == 0, cls.idx[1], cls.idx[0]).astype(np.int64)
    return idx, {"touched": _keep_class(level, cls, idx)}


def class_borders(level):
    b = [127, 128, -128, -129, 1919, 1920, -2176, -2177, 32639, 32640, 32767, -32768]
    return [7, 8, -8, -9] + b if level == 7 else b


def border(level, first, nrows):
    """quiet pairs (|idx| <= 3), ONE index per pair at a border between two width classes: the borders in turn, each in column 0 and in
    the last column, in the first and in the second row of its pair.  `first`: the stream's first (border, place) combination"""
    cols = 1 << level
    r, c = np.meshgrid(np.arange(nrows), np.arange(cols), indexing="ij")
    idx = ((5 * r + 3 * c) % 7 - 3).astype(np.int64)
    bs, want = class_borders(level), []
    for p in range(nrows // 2):
        k = first + p
        b, place = bs[k % len(bs)], (k // len(bs)) % 4
        idx[2 * p + (place >> 1), (cols - 1) * (place & 1)] = b
        want.append(expected_class(level, min(b, -3), max(b, 3)))
    return idx, {"pair_class": want}


def impulse(level, value, row, nrows):
    idx = np.zeros((nrows, 1 << level), dtype=np.int64)
    idx[row, (1 << level) // 3] = value
    return idx, {"row": row, "value": value}


def _code(block):
    """the narrowest linear filler (3..16 bits) that holds the block's indices; pwr = code - 1 is the smallest table that holds them"""
    return max(3, max(max(int(block.max()), 0).bit_length(), max(int(-block.min() - 1), 0).bit_length()) + 1)


def fast_value(level, val):
    """a header value the chunk kernel's fast path takes (mode_of: not silent, and below 2^16 as the levels from 10 on pre-scale it)"""
    return 0 < val < (1 << level if level >= 10 else 65536)


def craft(level, name, family, cls, height, content, ordinal):
    """`content(nrows)` as a stream of whole blocks of `height` rows, the fewest that hold four tiles of plan_rows(level) rows and one
    more row, less three samples.  Blocks of one row: four whole tiles and a ragged row; of three rows: up to two rows more; the tall
    blocks are two tiles high, so there are three of them - six tiles, the last one three samples short.
    Header values: header_values(level) in turn from the stream's ordinal on; a stream of tall blocks starts at one of the small values
    (1, 255, border - 1), so that at least its first block - whatever is added to or taken from the list of streams - is one the fast
    path of the chunk kernel takes (fast_value), and 65535, 0 and the border come behind them in turn"""
    pr = plan_rows(level)
    h = {"1": 1, "3": 3, "tall": 2 * pr}[height]
    nblocks = (4 * pr + 1 + h - 1) // h
    idx, meta = content(nblocks * h)
    assert idx.shape == (nblocks * h, 1 << level)
    vals, blocks = header_values(level), []
    if height == "tall":
        small = [i for i, v in enumerate(vals) if fast_value(level, v) and v < 65535]
        ordinal = small[ordinal % len(small)]
    for b in range(nblocks):
        rows = idx[b * h:(b + 1) * h]
        code = _code(rows)
        blocks.append((code - 1, vals[(b + ordinal) % len(vals)], code, rows))
    data = crafted_stream(level, h, blocks, cut=3)
    return Stream(name, family, cls, height, data, idx.astype(np.int16), np.array([(b[1], b[0]) for b in blocks], dtype=np.uint32), meta)


def variants(level):
    """[(name, family, class, content, every_height)]: every family x class in full; a variant is built at every block height
    (every_height) or at one, taken in turn, so that each family x class meets each height.  The aligned variants that attain a bound
    of a plane (both planes aligned or both reversed, at the outputs of bound_outputs) are built at every height: the streams of tall
    blocks take them down the chunk kernel's fast path, those of short blocks down its general path"""
    out = []
    G = stages(level)
    fams = level_families(level)
    for cls in level_classes(level):
        if "aligned" in fams:
            for n, q in enumerate(aligned_outputs(G)):
                attains = ("+0", "-0") if cls.hi is None else ("++", "--")
                if cls.hi is None:
                    combos = ["+0", "-0"]
                elif n == 0:
                    combos = ["++", "--", "+-", "-+", "+0", "-0", "0+", "0-"]
                else:
                    combos = ["++", "--"]
                for s in combos:
                    out.append(("aligned-%s-q%d%s" % (cls.name, q, s), "aligned", cls,
                                functools.partial(aligned, level, cls, q, s[0], s[1]),
                                (n == 0 and s in ("++", "--", "+0", "-0")) or (q in bound_outputs(G) and s in attains)))
        for end in (1, 0):
            out.append(("constant-%s-%s" % (cls.name, "max" if end else "min"), "constant", cls, functools.partial(constant, level, cls, end), True))
        for kind in ["col", "row"] + list(range(min(G, level))):
            out.append(("checker-%s-%s" % (cls.name, kind), "checker", cls, functools.partial(checker, level, cls, kind), kind == "col"))
        for value in ([cls.idx[1]] if cls.name == "wr" else [cls.idx[1], cls.idx[0]]):
            pr = plan_rows(level)
            for row in (0, 1, pr - 1, 4 * pr - 1):
                out.append(("impulse-%s-%d-row%d" % (cls.name, value, row), "impulse", cls, functools.partial(impulse, level, value, row), False))
    if "border" in fams:
        pairs, combos = 2 * plan_rows(level), 4 * len(class_borders(level))
        for t in range(max(3, (combos + pairs - 1) // pairs)):
            out.append(("border-%d" % t, "border", None, functools.partial(border, level, t * pairs), False))
    return out


@functools.lru_cache(None)
def level_streams(level):
    """every crafted stream of a level"""
    out, turn = [], 0
    for name, family, cls, content, every in variants(level):
        for height in (HEIGHTS if every else (HEIGHTS[turn % 3],)):
            out.append(craft(level, "%s-h%s" % (name, height), family, cls, height, content, len(out)))
        turn += not every
    return out


@functools.lru_cache(None)
def level_oracle(level):
    """[(PCM as uint16, status)] of the CPU oracle for level_streams(level): decoded once, shared by every test, read-only"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=8) as ex:
        out = list(ex.map(lambda s: oracle_pcm(s.data), level_streams(level)))
    for pcm, _ in out:
        pcm.flags.writeable = False
    return out
