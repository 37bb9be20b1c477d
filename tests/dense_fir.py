"""The model and the cases of dense crop batches with an overlay and impulse responses (acm_batch_decode_windows_overlay_fir,
include/acm_hip.h), for tests/test_dense_fir.py (the layout, the quantiser and the cases' own coverage, without a GPU) and
tests/test_gpu_dense_fir.py (the call itself).

A source row is tests/dense_overlay.py's; a filtered one is made from it by the contract's three lines on int64, channel by channel;
an output row is tests/dense_overlay.py's row_of over the rows the rest of the call sees.  The files are tests/dense_resample.py's
and one more, a full-scale stream of tests/extreme_content.py, which drives the accumulator to its bound."""
import functools

import numpy as np

import dense_crops as DC
import dense_overlay as DO
import dense_resample as DR
import extreme_content as EC
from libacm_amd import capi
from test_block_index import expected_window

RATE = DO.RATE
FRAMES = DO.FRAMES
TB = 64                                 # the kernel's tap block (tests/test_dense_fir.py holds it to the layout's own answer)
STAGE = 8 * TB                          # taps one fill of the kernel's LDS serves
MAX_L1 = 65535


# ---------------------------------------------------------------------------------------------------------------- the contract

def fir(x, h, d, s):
    """one channel: x int16 [T] -> (y int16 [T], acc int64 [T])"""
    T = x.size
    full = np.convolve(x.astype(np.int64), np.asarray(h, dtype=np.int64))       # full[m] = sum over t of h[t] * x[m - t], 0 <= m < T + ntaps - 1
    acc = np.zeros(T, dtype=np.int64)
    n = max(0, min(T, full.size - d))
    acc[:n] = full[d:d + n]
    y = np.clip((acc + ((1 << (s - 1)) if s else 0)) >> s, -32768, 32767).astype(np.int16)
    return y, acc


def channel(row, C, T, planar, ch):
    """the view of channel ch's T frames in a row of the batch's layout"""
    return row[ch * T:(ch + 1) * T] if planar or C == 1 else row[ch::C]


def filtered(row, C, T, planar, resp):
    """(F of the row, [acc of every channel]) for resp = (h, d, s)"""
    out, accs = np.empty_like(row), []
    for ch in range(C):
        y, acc = fir(channel(row, C, T, planar, ch), *resp)
        channel(out, C, T, planar, ch)[:] = y
        accs.append(acc)
    return out, accs


# ---------------------------------------------------------------------------------------------------------------- the files

_files = None


def files():
    """tests/dense_resample.py's, and behind them a mono stream at the batch's rate whose indices alternate between the ends of the
    whole range: half of its samples lie beyond +-16384"""
    global _files
    if _files is None:
        loud = EC.craft(5, "loud", "checker", EC.CLSWR, "tall", functools.partial(EC.checker, 5, EC.CLSWR, "col"), 0)
        _files = list(DR.files()) + [DC.File(loud.data)]
        assert len(_files) == LOUD_FILE + 1 and _files[-1].channels == 1 and _files[-1].info.rate == RATE and _files[-1].words >= 700
    return _files


LOUD_FILE = 12                          # the number of the loud file: tests/dense_resample.py has twelve


# ---------------------------------------------------------------------------------------------------------------- the cases

class Case(DO.Case):
    """DO.Case with `responses` [(h int16, d, s)] and `of_window` (a response number or None per window); a window may name LOUD_FILE"""

    def __init__(self, channels, frames, planar, windows, records, responses, of_window):
        super().__init__(channels, frames, planar, windows, records)
        self.responses, self.of_window = responses, of_window
        self._seen = self._accs = None

    def sources(self):
        """S: the source rows before any filter, int16 [nwin, R]; computed once, not to be written into"""
        if self._sources is None:
            src = []
            for (f, first, count), sp in zip(self.windows, self.speeds):
                if f == LOUD_FILE:
                    row = np.zeros((self.frames, self.channels), np.int16)
                    x = files()[f].pcm[first:first + count]
                    row[:x.size, :] = x[:, None]                # a mono file: with ACM_DENSE_MIX the sample goes into both channels
                    src.append(np.ascontiguousarray(row.T if self.planar else row).reshape(-1))
                else:
                    src.append(DO.DS.row_of(f, first, count, sp, self.channels, self.frames, self.planar, True, RATE))
            src = np.stack(src)
            src.setflags(write=False)
            self._sources = src
        return self._sources

    def seen(self):
        """what the rest of the call sees: F_k for a filtered window, S_k else; int16 [nwin, R].  accs(): {k: [acc per channel]}"""
        if self._seen is None:
            rows, self._accs = self.sources().copy(), {}
            for k, p in enumerate(self.of_window):
                if p is not None:
                    rows[k], self._accs[k] = filtered(self.sources()[k], self.channels, self.frames, self.planar, self.responses[p])
            rows.setflags(write=False)
            self._seen = rows
        return self._seen

    def accs(self):
        self.seen()
        return self._accs

    def rows(self):
        if self._rows is None:
            made = [DO.row_of(self.seen(), rec) for rec in self.records]
            out = np.stack([m[0] for m in made])
            out.setflags(write=False)
            self._rows = (out, [m[1] for m in made])
        return self._rows

    def expect(self, k):
        f, first, count = self.windows[k]
        if f == LOUD_FILE:
            return expected_window(files()[f].st, files()[f].rc, first, count)[:2]
        return super().expect(k)


(SPEECH, STEREO, UP, WIDE, DOWN, AWAY, BEHIND, CUT, UNUSED, BLOB, SHORT) = range(11)            # tests/dense_overlay.py's windows
LOUD, LOUD30, SAME0, SAME1, DRY = range(11, 16)                                                   # ... and this module's
(R_ONE, R_UNITY14, R_TWO, R_THREE, R_17, R_TB_LESS, R_TB, R_TB_MORE, R_LONG, R_SHIFT30, R_BOUND, R_STAGES, R_NOBODY) = range(13)


def _taps(rng, n, l1, decay):
    """n int16 taps of a decaying random shape, sum |h| at most l1 and close to it"""
    h = rng.standard_normal(n) * np.exp(-decay * np.arange(n) / n)
    q = np.trunc(h * (l1 / np.abs(h).sum())).astype(np.int64)
    assert np.abs(q).sum() <= l1 and np.abs(q).max() <= 32767
    return q.astype(np.int16)


def sign_matched(x, ntaps=257, peak=255):
    """(h, j0): h[t] = peak * sign(x[j0 - t]) - sum |h| = ntaps * peak - with j0 the output at which sum |x[j0 - t]| is largest, so
    acc[j0] = peak * sum |x[j0 - t]|: every product has one sign"""
    a = np.abs(x.astype(np.int64))
    j0 = int(np.convolve(a, np.ones(ntaps, np.int64))[:x.size].argmax())
    back = x[max(0, j0 - ntaps + 1):j0 + 1][::-1].astype(np.int64)               # x[j0 - t], t = 0 ..
    h = np.full(ntaps, peak, dtype=np.int64)
    h[:back.size] = np.where(back < 0, -peak, peak)
    return h.astype(np.int16), j0


def build_case(C, T, planar):
    base = DO.build_case(C, T, planar)
    L = files()[LOUD_FILE]
    loud = (LOUD_FILE, 0, min(T, L.words), None)
    windows = [w + (sp,) for w, sp in zip(base.windows, base.speeds)]
    windows += [loud, loud, windows[SPEECH], windows[SPEECH], windows[SPEECH]]
    assert len(windows) == DRY + 1
    rng = np.random.default_rng([0xF1E, C, T, int(planar)])
    x_loud = np.zeros(T, np.int16)
    x_loud[:loud[2]] = L.pcm[:loud[2]]
    responses = [None] * 13
    responses[R_ONE] = (np.array([1], np.int16), 0, 0)                            # the identity
    responses[R_UNITY14] = (np.array([16384], np.int16), 0, 14)                   # ... and again: the rounding bit changes nothing
    responses[R_TWO] = (np.array([20000, -12000], np.int16), 0, 15)
    responses[R_THREE] = (np.array([-5000, 30000, 7000], np.int16), 1, 15)
    responses[R_17] = (_taps(rng, 17, 50000, 2.0), 16, 15)                        # delay ntaps - 1: only inputs behind the output
    responses[R_TB_LESS] = (_taps(rng, TB - 1, 60000, 3.0), (TB - 1) // 2, 14)
    responses[R_TB] = (rng.integers(-3, 4, TB).astype(np.int16), 0, 0)            # shift 0, delay 0: the sums themselves, clamped
    responses[R_TB_MORE] = (_taps(rng, TB + 1, MAX_L1, 1.0), TB, 16)
    responses[R_LONG] = (_taps(rng, 8000, MAX_L1, 6.0), 4000, 13)                 # longer than any row: taps from both sides of [0, T)
    responses[R_SHIFT30] = (np.array([32767, 32767], np.int16), 0, 30)
    responses[R_BOUND] = (sign_matched(x_loud)[0], 0, 16)                         # sum |h| == 65535 over the loud row
    responses[R_STAGES] = (_taps(rng, 2 * STAGE + 76, 40000, 4.0), 300, 13)       # three fills of the LDS, the last one of two blocks
    responses[R_NOBODY] = (np.array([7] * 9, np.int16), 3, 2)                     # no window names it
    of_window = [None] * len(windows)
    for k, p in ((SPEECH, R_LONG), (STEREO, R_THREE), (UP, R_17), (DOWN, R_TB), (AWAY, R_TB_LESS), (BEHIND, R_TB_MORE), (CUT, R_STAGES),
                 (UNUSED, R_TWO), (BLOB, R_SHIFT30), (SHORT, R_LONG), (LOUD, R_BOUND), (LOUD30, R_SHIFT30), (SAME0, R_ONE), (SAME1, R_UNITY14)):
        of_window[k] = p                                                          # WIDE and DRY stay as they are
    N10 = DO.SNR10
    records = list(base.records)
    records += [(LOUD, None, 4096, 0, 0), (LOUD30, None, 4096, 0, 0), (SAME0, None, 4096, 0, 0), (SAME1, None, 4096, 0, 0), (DRY, None, 4096, 0, 0),
                (LOUD, UP, 4096, N10, 0), (WIDE, LOUD, 4096, N10, 0), (DRY, SPEECH, 2000, DO.SNR20, 0), (SHORT, SHORT, 4096, N10, 0),
                (WIDE, DRY, 4096, N10, 0), (SPEECH, WIDE, 3000, DO.SNR20, 0)]
    return Case(C, T, planar, windows, records, responses, of_window)


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = [build_case(c, t, planar) for c, planar in ((1, False), (2, False), (2, True)) for t in FRAMES]
    return _cases


def index():
    return DC.index_of(files())


def data():
    return [f.data for f in files()]
