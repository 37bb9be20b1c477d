"""The cases of dense crop batches over files of several sample rates (ACM_DENSE_RESAMPLE of acm_batch_decode_windows_dense,
include/acm_hip.h), for tests/test_dense_resample.py (the taps, the layout and the cases' own coverage, without a GPU) and
tests/test_gpu_dense_resample.py (the call itself).

Small files of their own at 11025, 22050, 44100 and 16000 Hz, mono and stereo, one at a rate whose table would be too large, one
whose header says rate 0 (no ACM file to the probe: the layout tests give the visitor an item of rate 0 instead), one blob that is not
ACM and one file cut off in its bytes.  A window is (file, first_word, max_words) in the file's OWN interleaved samples at its OWN rate.  What its row must hold is computed here from the oracle's whole-file decode: the
channel conversion of tests/dense_mix.py first, then the contract's filter, in numpy on integers (filter_frames); what it must report
comes from tests/test_block_index.py::expected_window, the rule the windows call is held to."""
from math import gcd

import numpy as np

import dense_crops as DC
from helpers import handmade_stream, make_stream
from libacm_amd import capi
from test_block_index import expected_window

RATE = 22050                    # the batch's
FRAMES = (64, 37, 2100)         # 2100: a row of two units, the second of which begins where the source base is no multiple of 8
Z = 8


# ---------------------------------------------------------------------------------------------------------------- the contract, in numpy

def ratio(rate_in, rate_out):
    """(L, M, K, Wd) of a supported ratio, else None"""
    if rate_in <= 0 or rate_out <= 0:
        return None
    g = gcd(rate_in, rate_out)
    L, M = rate_out // g, rate_in // g
    Wd = Z if L >= M else (Z * M + L - 1) // L
    return (L, M, 2 * Wd, Wd) if M <= 8 * L and L * 2 * Wd <= 16384 else None


def design(rate_in, rate_out):
    """the contract's taps: (L, M, K, Wd, q as int64 [L, K])"""
    L, M, K, Wd = ratio(rate_in, rate_out)
    s = min(1.0, L / M)
    ph, t = np.meshgrid(np.arange(L), np.arange(K), indexing="ij")
    u = ((t - Wd + 1) * L - ph) / L
    v = u * s / Z
    h = s * np.sinc(s * u) * np.where(np.abs(v) < 1, 0.5 + 0.5 * np.cos(np.pi * v), 0.0)
    h = h / h.sum(axis=1, keepdims=True)
    q = np.rint(h * 16384).astype(np.int64)
    q[np.arange(L), q.argmax(axis=1)] += 16384 - q.sum(axis=1)
    return L, M, K, Wd, q


_taps = {}


def taps(rate_in, rate_out):
    """the library's table for the ratio, what the kernel reads: (L, M, K, Wd, q as int64 [L, K]); asked for once"""
    key = (rate_in, rate_out)
    if key not in _taps:
        L, M, K, Wd, q = capi.dense_resample_taps(rate_in, rate_out)
        _taps[key] = (L, M, K, Wd, q.astype(np.int64))
    return _taps[key]


def n_out(f, L, M):
    return (f * L + M - 1) // M


def filter_frames(x, table):
    """one channel's source frames (after the channel conversion) -> (y int16 [n_out], acc int64 [n_out]): the contract's three lines"""
    L, M, K, Wd, q = table
    x = np.asarray(x, dtype=np.int64)
    f = x.size
    n = np.arange(n_out(f, L, M), dtype=np.int64) * M
    base, ph = n // L, n % L
    at = base[:, None] - Wd + 1 + np.arange(K)[None, :]
    inside = (at >= 0) & (at < f)
    xs = np.where(inside, x[np.clip(at, 0, max(f - 1, 0))] if f else 0, 0)
    acc = (q[ph] * xs).sum(axis=1)
    assert np.abs(acc).max(initial=0) < 2 ** 31
    return np.clip((acc + 8192) >> 14, -32768, 32767).astype(np.int16), acc


# ---------------------------------------------------------------------------------------------------------------- the files

_files = None


def files():
    global _files
    if _files is None:
        whole = make_stream(9411, 5, 16, 20, rate=44100)
        zero = handmade_stream(5, 16, [(9, 3000, 8)] * 6, rate=0, seed=94)
        _files = [DC.File(d) for d in (
            make_stream(9400, 5, 16, 20, rate=11025),                   # 0: up by 2: L = 2, M = 1, K = 16
            make_stream(9401, 5, 16, 20, channels=2, rate=11025),       # 1
            make_stream(9402, 5, 16, 20, rate=22050),                   # 2: the batch's own rate
            make_stream(9403, 5, 16, 20, channels=2, rate=22050),       # 3
            make_stream(9404, 5, 16, 20, rate=44100, cut=37),           # 4: down by 2: L = 1, M = 2, K = 32
            make_stream(9405, 5, 16, 20, channels=2, rate=44100),       # 5
            make_stream(9406, 5, 16, 20, rate=16000),                   # 6: L = 441, M = 320, K = 16: every phase is used
            make_stream(9407, 5, 16, 20, channels=2, rate=16000, cut=41),   # 7
            make_stream(9408, 5, 16, 20, rate=22051),                   # 8: a table of 22050 phases: not supported
            zero,                                                       # 9: the header says rate 0: the probe takes no such file for ACM
            b"not an acm file, whatever its length is",                 # 10
            whole[:len(whole) * 2 // 3],                                # 11: 44100, cut off in the middle of its bytes: an error end status
        )]
        assert [f.channels for f in _files] == [1, 2, 1, 2, 1, 2, 1, 2, 1, 0, 0, 1]
        assert [f.info.rate if f.acm else None for f in _files] == [11025, 11025, 22050, 22050, 44100, 44100, 16000, 16000, 22051, None, None, 44100]
        assert _files[11].end_status < 0 < _files[11].words and not _files[10].acm and not _files[9].acm
        assert [ratio(r, RATE) for r in (11025, 44100, 16000, 22051, 0)] == [(2, 1, 16, 8), (1, 2, 32, 16), (441, 320, 16, 8), None, None]
    return _files


def layout_item(f):
    """DC.layout_item with the header's rate"""
    it = DC.layout_item(f)
    it.info.rate = f.info.rate if f.acm else 0
    return it


def rate_of(f):
    """the rate of file f, None where it has none (not ACM, no such file)"""
    return files()[f].info.rate if f < len(files()) and files()[f].acm else None


def table_of(f, rate=RATE):
    """the library's table a window of file f is filtered by; None for a row that is not filtered - the batch's rate, no rate, a ratio
    that is not supported"""
    r = rate_of(f)
    return taps(r, rate) if r is not None and r != rate and ratio(r, rate) else None


def bad_ratio(f, rate=RATE):
    r = rate_of(f)
    return r is not None and r != rate and ratio(r, rate) is None


def chans_of(f, C):
    return files()[f].channels if f < len(files()) and files()[f].acm else C


def turned_away(f, C, mix, rate=RATE):
    """softly: another channel count without ACM_DENSE_MIX, or a ratio the filter does not take"""
    return (not mix and chans_of(f, C) != C) or bad_ratio(f, rate)


def delivered(f, first, count, C, mix, rate=RATE):
    """SOURCE samples a window delivers"""
    if f >= len(files()) or turned_away(f, C, mix, rate):
        return 0
    return max(0, min(count, files()[f].words - first))


def planes_of(f, first, words, C):
    """the window's source frames after the channel conversion: int64 [C, frames]"""
    src = files()[f].pcm[first:first + words].astype(np.int64)
    c = chans_of(f, C)
    if c == C:
        return src.reshape(-1, C).T
    if C == 1:
        return ((src[0::2] + src[1::2]) >> 1)[None, :]
    return np.stack([src, src])


def row_of(f, first, count, C, T, planar, mix, rate=RATE, acc=None):
    """the expected row, int16 [C * T]; acc (a list): the filter's sums of a filtered row are appended to it"""
    row = np.zeros((T, C), np.int16)
    words = delivered(f, first, count, C, mix, rate)
    if words:
        x = planes_of(f, first, words, C)
        table = table_of(f, rate)
        for ch in range(C):
            if table is None:
                y = x[ch]
            else:
                y, a = filter_frames(x[ch], table)
                if acc is not None:
                    acc.append(a)
            row[:y.size, ch] = y
    return np.ascontiguousarray(row.T if planar else row).reshape(-1)


def frames_out(f, first, count, C, mix, rate=RATE):
    """frames of the row that are the window's: n_out of a filtered one"""
    fr = delivered(f, first, count, C, mix, rate) // chans_of(f, C)
    table = table_of(f, rate)
    return n_out(fr, table[0], table[1]) if table is not None else fr


# ---------------------------------------------------------------------------------------------------------------- the cases

class Case:
    """one call with ACM_DENSE_RESAMPLE to RATE, with or without ACM_DENSE_MIX: `windows` over files() as rows of frames * channels"""

    def __init__(self, channels, frames, mix, windows):
        self.channels, self.frames, self.mix, self.windows = channels, frames, mix, windows
        self.row = channels * frames
        self.name = "c%d_t%d_%s" % (channels, frames, "mix" if mix else "plain")
        self._rows, self.accs = {}, []

    def filtered(self, k):
        f = self.windows[k][0]
        return table_of(f) is not None and not turned_away(f, self.channels, self.mix)

    def delivers(self, k):
        return delivered(*self.windows[k], self.channels, self.mix)

    def frames_out(self, k):
        return frames_out(*self.windows[k], self.channels, self.mix)

    def expect(self, k):
        """(words, status, blocks staged) the call reports for window k: acm_batch_decode_windows' own unless it is turned away"""
        f, first, count = self.windows[k]
        if f >= len(files()) or turned_away(f, self.channels, self.mix):
            return 0, capi.ERR_ARG, 0
        words, status, b0, nb = expected_window(files()[f].st, files()[f].rc, first, count)
        return words, status, nb

    def rows(self, planar):
        """the expected tensor, int16 [N, row]; computed once, not to be written into"""
        if planar not in self._rows:
            acc = [] if not self._rows else None
            out = np.stack([row_of(f, first, count, self.channels, self.frames, planar, self.mix, acc=acc) for f, first, count in self.windows])
            out.setflags(write=False)
            self._rows[planar] = out
            if acc is not None:
                self.accs = acc
        return self._rows[planar]


def longest(f, T):
    """frames of the longest window of file f that fits a row: T * M // L where it is filtered, else T"""
    table = table_of(f)
    return T * table[1] // table[0] if table is not None else T


def _windows_of(f, T, rng):
    """the windows of one ACM file that is not turned away for its channel count, in the file's own samples"""
    src = files()[f]
    c, W, bl = src.channels, src.words, src.st.block_len
    F = longest(f, T)
    table = table_of(f)
    Wd = table[3] if table is not None else Z
    assert W > 8 * 11 + F * c + 8
    wins = [(f, 8 * (3 + r) + r, F * c) for r in range(0, 8, c)]                    # every residue of first_word % 8 a multiple of c can have
    wins += [(f, 5 * c, 0), (f, 6 * c, c), (f, 11 * c, 2 * c), (f, 4 * c, (Wd - 1) * c),   # nothing, 1 and 2 frames, shorter than the filter
             (f, 17 * c, (F - 1) * c), (f, 9 * c, F * c)]                           # a full row, and one frame fewer
    wins += [(f, W + 3 * c, 4 * c),                                                 # starts behind the end
             (f, W - 5 * c, F * c),                                                 # clipped by the end
             (f, bl - 3 * c, 8 * c)]                                                # across a block boundary
    for _ in range(2):
        n = int(rng.integers(1, F + 1))
        wins.append((f, c * int(rng.integers(0, W // c - n + 1)), c * n))
    return wins


def build_case(C, T, mix):
    rng = np.random.default_rng([0x5A3E, C, T, int(mix)])
    same, other = [], []
    for f, src in enumerate(files()):
        if not src.acm:
            continue
        c = src.channels
        if c != C and not mix:                                                      # turned away: checked as a row of C channels at RATE
            wins = [(f, 8 * C, T * C), (f, 2 * C, 0), (f, 4 * C, 6 * C)]
        elif f == 11:                                                               # the file that breaks off: its own status at the end
            W, F = src.words, longest(f, T)
            wins = [(11, 3, F), (11, max(W - 2 * F, 0) // 8 * 8 + 5, F), (11, W - 8, F), (11, W + 1, 4), (11, 12, 9)]
        else:
            wins = _windows_of(f, T, rng)
        (other if table_of(f) is not None else same).extend(wins)
    # consecutive rows alternate between rows at the batch's rate and filtered ones, as long as both last
    wins = [w for pair in zip(same, other) for w in pair]
    rest = same[len(other):] + other[len(same):]
    extra = [(10, 0, C * T), (10, 4 * C, 0), (99, 0, 4 * C), (9, 8 * C, C * T)]     # not ACM, no such file, rate 0: checked against C and RATE
    for k, w in enumerate(extra):
        rest.insert(3 * k + 1, w)
    return Case(C, T, mix, wins + rest)


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = [build_case(c, t, mix) for mix in (True, False) for c in (1, 2) for t in FRAMES]
    return _cases
