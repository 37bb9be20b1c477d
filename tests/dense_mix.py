"""The cases of dense crop batches over files of both channel counts (ACM_DENSE_MIX of acm_batch_decode_windows_dense, include/acm_hip.h),
for tests/test_dense_mix.py (the layout, the cases' own coverage and the kernel's code, without a GPU) and tests/test_gpu_dense_mix.py
(the call itself).

The files are tests/dense_crops.py's.  A window is (file, first_word, max_words) in the file's OWN interleaved samples, whatever the
batch's channel count; what its row must hold is computed here from the oracle's whole-file decode by the contract's table, in numpy,
and what it must report comes from tests/test_block_index.py::expected_window, the rule the windows call is held to."""
import numpy as np

import dense_crops as DC
from libacm_amd import capi
from test_block_index import expected_window

FRAMES = DC.FRAMES
COPY, SPLIT, DOWN, UP_INTER, UP_PLANAR = range(5)       # AcmDenseMode (libacm_amd/csrc/acm_device.h)
MODE_SHIFT = 56                                         # ACM_DENSE_MODE_SHIFT
ODD_SHIFT = 1                                           # elements behind a 16-byte line at which one GPU test lets its tensor begin
files = DC.files


def head_of(k, row, unit, shift):
    """elements of row k in front of its first 16-byte line, as the kernels cut a row, for a tensor of `unit`-byte elements that begins
    `shift` elements plus a guard row of `row` elements behind a 256-byte aligned base (the buffers of the GPU tests)"""
    at = (row + shift + k * row) * unit
    return min((-at & 15) // unit, row)


def chans_of(f, C):
    """samples per frame of a window of file f in a batch of C channels: the file's own, C where it has none"""
    return files()[f].channels if f < len(files()) and files()[f].acm else C


def mode_of(f, C, planar):
    c = chans_of(f, C)
    if c == C:
        return SPLIT if C == 2 and planar else COPY
    return DOWN if C == 1 else UP_PLANAR if planar else UP_INTER


def delivered(f, first, count):
    """samples of `whole` a window holds: none of a file that is not ACM or of no file at all"""
    if f >= len(files()):
        return 0
    return max(0, min(count, files()[f].words - first))


def row_of(f, first, count, C, T, planar):
    """the expected row, int16 [C * T]: the contract's table, vectorised"""
    row = np.zeros(C * T, np.int16)
    words = delivered(f, first, count)
    if not words:
        return row
    src = files()[f].pcm[first:first + words]
    c = chans_of(f, C)
    if c == C:
        row[:words] = src
        return np.ascontiguousarray(row.reshape(T, C).T).reshape(-1) if planar else row
    if C == 1:
        pairs = src[:words // 2 * 2].astype(np.int32).reshape(-1, 2)
        row[:words // 2] = (pairs[:, 0] + pairs[:, 1]) >> 1
    elif planar:
        row[:words] = row[T:T + words] = src
    else:
        row[0:2 * words:2] = row[1:2 * words:2] = src
    return row


def sums(f):
    """L + R of every frame of a stereo file, in 32 bits"""
    p = files()[f].pcm.astype(np.int32)
    return p[0::2] + p[1::2]


SUM_KINDS = {"an odd negative sum": lambda s: (s < 0) & (s % 2 != 0), "an odd positive sum": lambda s: (s > 0) & (s % 2 != 0),
             "a sum beyond int16": lambda s: abs(s) > 32767}


class Case:
    """one call with ACM_DENSE_MIX: `windows` over files() as rows of frames * channels samples"""

    def __init__(self, channels, frames, windows):
        self.channels, self.frames, self.windows = channels, frames, windows
        self.row = channels * frames
        self.name = "c%d_t%d" % (channels, frames)
        self._rows = {}

    def mode(self, k, planar):
        return mode_of(self.windows[k][0], self.channels, planar)

    def delivers(self, k):
        return delivered(*self.windows[k])

    def frames_delivered(self, k):
        return self.delivers(k) // chans_of(self.windows[k][0], self.channels)

    def expect(self, k):
        """(words, status, blocks staged) the call reports for window k: acm_batch_decode_windows' own"""
        f, first, count = self.windows[k]
        if f >= len(files()):
            return 0, capi.ERR_ARG, 0
        words, status, b0, nb = expected_window(files()[f].st, files()[f].rc, first, count)
        return words, status, nb

    def rows(self, planar):
        """the expected tensor, int16 [N, row]; computed once, not to be written into"""
        if planar not in self._rows:
            out = np.stack([row_of(f, first, count, self.channels, self.frames, planar) for f, first, count in self.windows])
            out.setflags(write=False)
            self._rows[planar] = out
        return self._rows[planar]


def _windows_of(f, C, T, rng):
    """the windows of one ACM file in a batch of C channels and T frames, in the file's own samples"""
    src = files()[f]
    c, W, bl = src.channels, src.words, src.st.block_len
    assert W > 8 * 11 + T * c + 8
    wins = [(f, 8 * (3 + r) + r, T * c) for r in range(0, 8, c)]                    # every residue of first_word % 8 a multiple of c can have
    wins += [(f, 5 * c, 0), (f, 6 * c, c), (f, 11 * c, 7 * c), (f, 4 * c, 8 * c), (f, 13 * c, 9 * c), (f, 17 * c, (T - 1) * c), (f, 9 * c, T * c)]
    wins += [(f, W + 3 * c, 4 * c),                                                 # starts behind the end
             (f, W - 5 * c, T * c),                                                 # clipped by the end
             (f, bl - 3 * c, 8 * c)]                                                # across a block boundary
    if c == 2 and C == 1:                                                           # frames whose down-mix tells the laws apart, inside a window
        s = sums(f)
        for kind in SUM_KINDS.values():
            at = int(np.nonzero(kind(s))[0][0])
            wins.append((f, 2 * max(at - 3, 0), 2 * 9))
    for _ in range(4):
        n = int(rng.integers(1, T + 1))
        wins.append((f, c * int(rng.integers(0, W // c - n + 1)), c * n))
    return wins


def build_case(C, T):
    rng = np.random.default_rng([0xD1C5, C, T])
    same, other = [], []
    for f, src in enumerate(files()):
        if not src.acm:
            continue
        if f == 6:                                                                  # the file that breaks off: its own status at the end
            W = src.words
            wins = [(6, 3, T), (6, W - 8, T), (6, W + 1, 4), (6, 12, 9)]
        else:
            wins = _windows_of(f, C, T, rng)
        (same if src.channels == C else other).extend(wins)
    # consecutive rows alternate between the plain mode and the converting one, as long as both last
    wins = [w for pair in zip(same, other) for w in pair]
    rest = same[len(other):] + other[len(same):]
    extra = [(7, 0, C * T), (7, 4 * C, 0), (99, 0, 4 * C)]                          # not ACM, no such file: checked against C, rows of zeros
    for k, w in enumerate(extra):                                                   # ... among the rows that remain
        rest.insert(3 * k + 1, w)
    return Case(C, T, wins + rest)


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = [build_case(c, t) for c in (1, 2) for t in FRAMES]
    return _cases


def model(items, wins, frames, channels, planar, parse, f32, final_words=None):
    """the visitor's tables of an accepted call with ACM_DENSE_MIX, as acm_dense_layout.h words them.  items: DC.layout_item per file"""
    import test_dense_crops as TD
    import test_window_layout as WL
    R = frames * channels
    lay = WL.model(WL.Case("", items, wins, parse=parse))
    assert lay["totals"]["rc"] == 0
    report, rows, modes = [], [], []
    for k, s in enumerate(lay["slots"]):
        f = wins[k][0]
        has = f < len(items) and bool(items[f].ok)
        c = items[f].info.channels if has else channels
        mode = (SPLIT if channels == 2 and planar else COPY) if c == channels else DOWN if channels == 1 else UP_PLANAR if planar else UP_INTER
        modes.append(mode)
        report.append((s["status"], s["words"], k * R, k * R, R))
        count = min(s["words"], s["words"] if final_words is None else final_words[k]) if s["active"] else 0
        rows.append((s["dev_off"], count | (mode << MODE_SHIFT if mode >= DOWN else 0)) if count else (0, 0))
    t = lay["totals"]
    tot = dict(frames=frames, row_words=R, channels=channels, planar=int(planar), f32=int(f32), out_words=len(wins) * R,
               pcm_arena_words=t["pcm_total"] + TD.PCM_SLACK, blocks_parsed=t["blocks_parsed"],
               table_off=WL.round_up(t["jobs_bytes"] + t["bjobs_bytes"] + t["res_bytes"], 64), table_bytes=16 * len(wins), rc=0)
    converts = int(any(count >> MODE_SHIFT for _, count in rows))
    return {"wins": [tuple(w) for w in wins], "rejected": [0] * len(wins), "report": report, "rows": rows, "mix": modes + [converts], "totals": tot}
