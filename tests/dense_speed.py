"""The cases of dense crop batches with a speed per window (ACM_DENSE_SPEED of acm_batch_decode_windows_dense, include/acm_hip.h), for
tests/test_dense_speed.py (the tables, the classification, the layout and the cases' own coverage, without a GPU) and
tests/test_gpu_dense_speed.py (the call itself).

The files are tests/dense_resample.py's.  A window is (file, first_word, max_words, speed) in the file's OWN interleaved samples at its
OWN rate, speed None or (num, den).  What its row must hold is computed here from the oracle's whole-file decode: the channel
conversion of tests/dense_mix.py first, then - by the contract's classification - nothing, the exact filter
(dense_resample.filter_frames) or the wide one, in numpy on int64 (wide_frames); what it must report comes from
tests/test_block_index.py::expected_window, the rule the windows call is held to."""
from math import gcd

import numpy as np

import dense_resample as DR
from libacm_amd import capi
from test_block_index import expected_window

RATE = DR.RATE                  # the batch's, but for the steepest cases
FRAMES = (64, 37, 2100)         # 2100: a row of two units
Z = 8
SPAN_CAP, UNIT = 15872, 2048    # acm_dense_filter.h: samples of the staged planes, outputs of a unit


# ---------------------------------------------------------------------------------------------------------------- the contract, in numpy

class Filter:
    """what a row of a file at rate_in played at num / den gets in a batch at rate_out: kind "none", "exact", "wide" or "bad" and the
    contract's numbers for it"""

    def __init__(self, rate_in, rate_out, speed=None):
        num, den = speed or (1, 1)
        self.kind, self.key = "bad", None
        if not rate_in or not rate_out or not 0 < num < 65536 or not 0 < den < 65536:
            return
        g = gcd(rate_in * num, rate_out * den)
        self.L, self.M = L, M = rate_out * den // g, rate_in * num // g
        Wd = Z if L >= M else -(-Z * M // L)
        if L == M:
            self.kind = "none"
        elif M > 8 * L:
            pass
        elif L * 2 * Wd <= 16384:
            self.kind, self.K, self.Wd, self.key = "exact", 2 * Wd, Wd, (L, M)
        elif L < 2 ** 31 and M < 2 ** 31:
            self.kind = "wide"
            self.c = 64 if L >= M else 64 * L // M
            self.K, self.Wd, self.P, self.b = wide_shape(self.c)
            self.step = (M << 32) // L
            self.key = self.c

    def n_out(self, f):
        return f if self.kind == "none" else -(-f * self.L // self.M)

    def longest(self, T):
        """source frames of the longest window that fits a row of T frames"""
        return T if self.kind in ("none", "bad") else T * self.M // self.L


def wide_shape(c):
    """(K, Wd, P, b) of the wide table of cutoff c"""
    Wd = Z if c == 64 else -(-64 * Z // c)
    K = 2 * Wd
    b = 0
    while ((2 << b) + 1) * K <= 16384:
        b += 1
    return K, Wd, 1 << b, b


def design_wide(c):
    """the contract's wide taps: q as int64 [P + 1, K]"""
    K, Wd, P, b = wide_shape(c)
    s = c / 64
    p, t = np.meshgrid(np.arange(P + 1), np.arange(K), indexing="ij")
    u = (t - Wd + 1) - p / P
    v = u * s / Z
    h = s * np.sinc(s * u) * np.where(np.abs(v) < 1, 0.5 + 0.5 * np.cos(np.pi * v), 0.0)
    h = h / h.sum(axis=1, keepdims=True)
    q = np.rint(h * 16384).astype(np.int64)
    q[np.arange(P + 1), q.argmax(axis=1)] += 16384 - q.sum(axis=1)
    return q


def wide_positions(flt, n):
    """(base, p, w, frac) of output frames 0 .. n - 1, int64 each"""
    assert n < 2 ** 28 and flt.step < 2 ** 36
    X = np.arange(n, dtype=np.uint64) * np.uint64(flt.step)
    base = (X >> np.uint64(32)).astype(np.int64)
    frac = (X & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return base, frac >> (32 - flt.b), (frac >> (17 - flt.b)) & 32767, frac


def wide_frames(x, flt, q):
    """one channel's source frames (after the channel conversion) -> y int16 [n_out]: the contract's lines on int64"""
    x = np.asarray(x, dtype=np.int64)
    f = x.size
    base, p, w, _ = wide_positions(flt, flt.n_out(f))
    at = base[:, None] - flt.Wd + 1 + np.arange(flt.K)[None, :]
    inside = (at >= 0) & (at < f)
    xs = np.where(inside, x[np.clip(at, 0, max(f - 1, 0))] if f else 0, 0)
    a0, a1 = (q[p] * xs).sum(axis=1), (q[p + 1] * xs).sum(axis=1)
    assert max(np.abs(a0).max(initial=0), np.abs(a1).max(initial=0)) < 2 ** 31
    acc = a0 + (((a1 - a0) * w) >> 15)
    return np.clip((acc + 8192) >> 14, -32768, 32767).astype(np.int16)


_tables = {}


def table(rate_in, rate_out, speed=None):
    """(Filter, the library's table for it as int64 [phases, K] - what the kernel reads; None where the row is not filtered); a table
    is asked for once per (L, M) or c"""
    flt = Filter(rate_in, rate_out, speed)
    if flt.key is None:
        return flt, None
    if flt.key not in _tables:
        info, q = capi.dense_speed_taps(rate_in, rate_out, speed or (1, 1))
        assert capi.SPEED_KINDS[info.kind] == flt.kind
        _tables[flt.key] = q.astype(np.int64)
    return flt, _tables[flt.key]


def resample(x, flt, q):
    if flt.kind == "exact":
        return DR.filter_frames(x, (flt.L, flt.M, flt.K, flt.Wd, q))[0]
    return wide_frames(x, flt, q)


# ---------------------------------------------------------------------------------------------------------------- rows

def filter_of(f, rate, speed):
    """(Filter, table) of a window of file f; kind "none" for a file without a rate: it is checked as a row of the batch's own"""
    r = DR.rate_of(f)
    return table(r, rate, speed) if r is not None else (Filter(rate, rate), None)


def turned_away(f, C, mix, rate, speed):
    """softly: another channel count without ACM_DENSE_MIX, or a ratio neither filter takes"""
    if not mix and DR.chans_of(f, C) != C:
        return True
    return filter_of(f, rate, speed)[0].kind == "bad"


def delivered(f, first, count, speed, C, mix, rate):
    """SOURCE samples a window delivers"""
    if f >= len(DR.files()) or turned_away(f, C, mix, rate, speed):
        return 0
    return max(0, min(count, DR.files()[f].words - first))


def row_of(f, first, count, speed, C, T, planar, mix, rate):
    """the expected row, int16 [C * T]"""
    row = np.zeros((T, C), np.int16)
    words = delivered(f, first, count, speed, C, mix, rate)
    if words:
        x = DR.planes_of(f, first, words, C)
        flt, q = filter_of(f, rate, speed)
        for ch in range(C):
            y = x[ch] if q is None else resample(x[ch], flt, q)
            row[:y.size, ch] = y
    return np.ascontiguousarray(row.T if planar else row).reshape(-1)


class Case:
    """one call with ACM_DENSE_RESAMPLE | ACM_DENSE_SPEED to `rate`, with or without ACM_DENSE_MIX"""

    def __init__(self, channels, frames, mix, windows, rate=RATE, tag=""):
        self.channels, self.frames, self.mix, self.rate = channels, frames, mix, rate
        self.windows = [w[:3] for w in windows]
        self.speeds = [w[3] for w in windows]
        self.row = channels * frames
        self.name = "%sc%d_t%d_%s" % (tag, channels, frames, "mix" if mix else "plain")
        self._rows = {}

    def filter(self, k):
        """the Filter of window k; None where the window is turned away or has no file"""
        f = self.windows[k][0]
        if f >= len(DR.files()) or turned_away(f, self.channels, self.mix, self.rate, self.speeds[k]):
            return None
        return filter_of(f, self.rate, self.speeds[k])[0]

    def delivers(self, k):
        return delivered(*self.windows[k], self.speeds[k], self.channels, self.mix, self.rate)

    def frames_in(self, k):
        return self.delivers(k) // DR.chans_of(self.windows[k][0], self.channels)

    def frames_out(self, k):
        flt = self.filter(k)
        return flt.n_out(self.frames_in(k)) if flt else 0

    def expect(self, k):
        """(words, status, blocks staged) the call reports for window k: acm_batch_decode_windows' own unless it is turned away"""
        f, first, count = self.windows[k]
        if f >= len(DR.files()) or turned_away(f, self.channels, self.mix, self.rate, self.speeds[k]):
            return 0, capi.ERR_ARG, 0
        words, status, b0, nb = expected_window(DR.files()[f].st, DR.files()[f].rc, first, count)
        return words, status, nb

    def rows(self, planar):
        """the expected tensor, int16 [N, row]; computed once, not to be written into"""
        if planar not in self._rows:
            out = np.stack([row_of(*w, sp, self.channels, self.frames, planar, self.mix, self.rate) for w, sp in zip(self.windows, self.speeds)])
            out.setflags(write=False)
            self._rows[planar] = out
        return self._rows[planar]


# ---------------------------------------------------------------------------------------------------------------- the cases

NEAR_ONE = (29999, 30000)       # upsampling by a hair: frame 1 lies 1 / 30000 in front of source frame 1 - the last phase pair, w above 32000
POWER_OF_TWO = (2047, 2048)     # L = 2048: the step is exact, and frame 2048 lies on a source frame again - frac == 0 behind frame 0
SPEEDS = {11025: [None, NEAR_ONE, (1001, 1000), (9, 10)],
          22050: [None, NEAR_ONE, (1001, 1000), (9, 10), (11, 10), (2, 2), POWER_OF_TWO],
          44100: [None, NEAR_ONE, (1001, 1000)],
          16000: [None, NEAR_ONE, (9, 10)],
          22051: [None, (9, 10)]}


def build_case(C, T, mix):
    rng = np.random.default_rng([0x5BEED, C, T, int(mix)])
    wins = []
    for f, src in enumerate(DR.files()):
        if not src.acm:
            continue
        c, W = src.channels, src.words
        if c != C and not mix:                          # turned away for its channel count: checked as a row of C channels at RATE
            wins += [(f, 8 * C, T * C, None), (f, 4 * C, 6 * C, (11, 10))]
            continue
        speeds = SPEEDS[src.info.rate] if f != 11 else [None, (1001, 1000)]
        for i, sp in enumerate(speeds):
            F = Filter(src.info.rate, RATE, sp).longest(T)
            assert W > (8 * 9 + 9) * c + F * c
            wins += [(f, (8 * (i + 1) + 2 * i + 1) * c, F * c, sp),                 # a full row, from every residue of first_word % 8
                     (f, (3 + i) * c, (F - 1) * c, sp),
                     (f, c * int(rng.integers(0, W // c - F)), c * int(rng.integers(1, F + 1)), sp)]
            if i < 2:
                wins += [(f, 5 * c, 0, sp), (f, 6 * c, c, sp), (f, W - 5 * c, F * c, sp), (f, W + 3 * c, 4 * c, sp)]
    # ratios beyond an eighth, no file, no ACM file, a rate of 0: rows of zeros among the others
    away = (4, 2) if C == 1 else (5, 3)                 # (a window counts its file's own samples: T frames of the file's channel count)
    extra = [(away[0], 8 * C, T * C, (5, 1)), (10, 0, C * T, (9, 10)), (99, 0, 4 * C, None), (9, 8 * C, C * T, (11, 10)),
             (away[1], 16 * C, 2 * C, (9, 1))]
    for k, w in enumerate(extra):
        wins.insert(7 * k + 3, w)
    return Case(C, T, mix, wins)


STEEP_RATE, STEEP_T = 2050, 1100


def build_steep_case(C):
    """16000 Hz played at 999 / 1000 into a batch at 2050 Hz: L = 1025, M = 7992, c = 8, K = 128 - the most source an output can need,
    so a unit of a mono row or a plane takes two passes; beside it the exact rows of 16000 and 11025 Hz and files that are turned away"""
    sp = (999, 1000)
    F = Filter(16000, STEEP_RATE, sp).longest(STEEP_T)
    assert F == 8576
    wins = [(6, 3, F, sp), (2, 8, 64, None), (0, 5, 5000, None), (6, 1001, F - 1, sp), (7, 2, 2 * 4100, sp), (6, 16, 8193, None), (4, 0, 8, sp),
            (1, 6, 2 * 2000, sp), (6, 40, 63, sp), (7, 8, 2 * 4000, None), (6, 24, 8100, sp)]
    return Case(C, STEEP_T, True, wins, rate=STEEP_RATE, tag="steep_")


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = [build_case(c, t, mix) for mix in (True, False) for c in (1, 2) for t in FRAMES] + [build_steep_case(c) for c in (1, 2)]
    return _cases


def passes_of_a_unit(flt, epf):
    """how many passes the kernel takes for a full unit of a wide row with epf elements a frame: the planes hold SPAN_CAP samples"""
    P = UNIT
    while epf * ((((P + 16) // epf * flt.step) >> 32) + 1 + flt.K + 2) > SPAN_CAP:
        P >>= 1
    return UNIT // P
