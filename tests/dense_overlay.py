"""The model and the cases of dense crop batches with an overlay (acm_batch_decode_windows_overlay, include/acm_hip.h), for
tests/test_dense_overlay.py (the gain, the layout and the cases' own coverage, without a GPU) and tests/test_gpu_dense_overlay.py (the
call itself).

The files are tests/dense_resample.py's and a source row is tests/dense_speed.py's row_of - the row acm_batch_decode_windows_dense
writes for a window with ACM_DENSE_MIX, ACM_DENSE_RESAMPLE and ACM_DENSE_SPEED set, which the existing tests hold to their own models.
An output row is made from two of them by the contract's lines: the gain on Python integers, the rest on int64."""
from math import isqrt

import numpy as np

import dense_resample as DR
import dense_speed as DS
from libacm_amd import batch, capi
from test_block_index import expected_window

RATE = DR.RATE
FRAMES = (1, 37, 64, 2100, 6151)        # 6151: three units and seven - an energy summed by four workgroups, and odd
G_MAX = 32768
NONE = None                             # b of a row with nothing laid over it


# ---------------------------------------------------------------------------------------------------------------- the contract

def gain(ea, eb, snr):
    """g of SNR mode, on unbounded integers"""
    D = eb * snr
    return 0 if D == 0 else min(G_MAX, isqrt((ea << 40) // D))


def energy(row):
    return int((row.astype(np.int64) ** 2).sum())


def products(A, B, g, vol):
    """m * vol + 2^23 of every element, int64"""
    m = 4096 * A.astype(np.int64) + g * B.astype(np.int64)
    assert np.abs(m).max(initial=0) <= 2 ** 27 + 2 ** 30
    return m * (vol or 4096) + (1 << 23)


def combine(A, B, g, vol):
    return np.clip(products(A, B, g, vol) >> 24, -32768, 32767).astype(np.int16)


def row_of(sources, rec):
    """(the output row int16 [R], (g, energy_a, energy_b) as the call reports them) of record (a, b, vol, snr, gain)"""
    a, b, vol, snr, g = rec[:5]
    A = sources[a]
    if b is None:
        return combine(A, np.zeros_like(A), 0, vol), (0, 0, 0)
    B = sources[b]
    if snr == 0:
        return combine(A, B, g, vol), (g, 0, 0)
    ea, eb = energy(A), energy(B)
    g = gain(ea, eb, snr)
    return combine(A, B, g, vol), (g, ea, eb)


# ---------------------------------------------------------------------------------------------------------------- the cases

class Case:
    """one call: `windows` (file, first_word, max_words) with `speeds` over DR.files() as source rows of frames * channels, mixed,
    resampled to RATE and played at their speeds; `records` (a, b, vol, snr, gain) as output rows"""

    def __init__(self, channels, frames, planar, windows, records):
        self.channels, self.frames, self.planar = channels, frames, planar
        self.windows = [w[:3] for w in windows]
        self.speeds = [w[3] for w in windows]
        self.records = records
        self.row = channels * frames
        self.name = "c%d_t%d_%s" % (channels, frames, "planar" if planar else "inter")
        self._sources = self._rows = None

    def sources(self):
        """the source rows, int16 [nwin, R]; computed once, not to be written into"""
        if self._sources is None:
            src = np.stack([DS.row_of(*w, sp, self.channels, self.frames, self.planar, True, RATE) for w, sp in zip(self.windows, self.speeds)])
            src.setflags(write=False)
            self._sources = src
        return self._sources

    def rows(self):
        """(the expected tensor int16 [nrows, R], [(g, energy_a, energy_b)]); computed once"""
        if self._rows is None:
            made = [row_of(self.sources(), rec) for rec in self.records]
            out = np.stack([m[0] for m in made])
            out.setflags(write=False)
            self._rows = (out, [m[1] for m in made])
        return self._rows

    def expect(self, k):
        """(words, status) the call reports for window k: the dense call's"""
        f, first, count = self.windows[k]
        if f >= len(DR.files()) or DS.turned_away(f, self.channels, True, RATE, self.speeds[k]):
            return 0, capi.ERR_ARG
        words, status, b0, nb = expected_window(DR.files()[f].st, DR.files()[f].rc, first, count)
        return words, status


SPEECH, STEREO, UP, WIDE, DOWN, AWAY, BEHIND, CUT, UNUSED, BLOB, SHORT = range(11)       # the source rows of every case
SNR10, SNR20, SNR_5 = batch.snr_q16(10), batch.snr_q16(20), batch.snr_q16(-5)


def build_case(C, T, planar):
    def win(f, first, speed, frames=None):
        """a window of file f from frame `first` on, as long as a row takes (or `frames`), in the file's own samples"""
        c = DR.files()[f].channels
        F = DS.Filter(DR.rate_of(f), RATE, speed).longest(T) if frames is None else frames
        return (f, first * c, F * c, speed)
    W = DR.files()[2].words
    windows = [win(2, 8, None),                         # SPEECH: the batch's own rate, mono
               win(3, 5, None),                         # STEREO: ... stereo
               win(0, 3, None),                         # UP: 11025 Hz, the exact filter
               win(6, 11, DS.NEAR_ONE),                 # WIDE: 16000 Hz a hair slower, the wide filter
               win(5, 2, (1001, 1000)),                 # DOWN: 44100 Hz stereo, the wide filter downwards
               win(4, 8, (5, 1), T),                    # AWAY: a ratio beyond an eighth - turned away, a row of zeros
               (2, W + 3, min(4, T), None),             # BEHIND: behind its stream's end - delivers nothing
               win(7, 4, None),                         # CUT: 16000 Hz stereo, a file that breaks off
               win(1, 6, (9, 10)),                      # UNUSED: no row names it
               (10, 0, T * C, None),                    # BLOB: not an ACM file
               win(2, 40, None, T // 4)]                # SHORT: a quarter of a row, zeros behind it - what is made loud clamps there alone
    assert len(windows) == SHORT + 1
    records = [(SPEECH, NONE, 4096, 0, 0), (SPEECH, NONE, 2048, 0, 0), (SHORT, NONE, 65535, 0, 0),         # volume alone
               (STEREO, STEREO, 0, SNR10, 0),                                                             # a == b, vol 0 is 4096
               (SPEECH, UP, 4096, SNR10, 0), (STEREO, UP, 4096, SNR20, 0), (WIDE, UP, 5000, 2 ** 32 - 1, 0), (DOWN, UP, 3000, SNR_5, 0),
               (STEREO, SHORT, 4096, 1, 0),                                                               # snr 1: g at G_MAX
               (SPEECH, AWAY, 4096, SNR10, 0),                                                            # Eb == 0
               (BEHIND, SPEECH, 4096, SNR10, 0),                                                          # Ea == 0
               (WIDE, DOWN, 4096, 0, 0), (CUT, SHORT, 4096, 0, 32768), (UP, CUT, 7000, 0, 1234),          # absolute gains
               (BLOB, SPEECH, 4096, SNR20, 0), (CUT, STEREO, 5000, SNR20, 0), (UP, DOWN, 1, SNR10, 0)]
    records += [(k, NONE, 4096, 0, 0) for k in reversed(range(len(windows))) if k != UNUSED]             # the identity, in reverse order
    return Case(C, T, planar, windows, records)


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = [build_case(c, t, planar) for c, planar in ((1, False), (2, False), (2, True)) for t in FRAMES]
    return _cases
