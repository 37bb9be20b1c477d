"""The model and the cases of mel filterbank features from dense crop batches (acm_batch_decode_windows_features, include/acm_hip.h),
for tests/test_dense_feat.py (the design, the check, the cases' own coverage and the model against a float64 spectrogram, without a
GPU) and tests/test_gpu_dense_feat.py (the call itself).

An output row Y_r is tests/dense_fir.py's - the int16 row acm_batch_decode_windows_overlay_fir writes for the same windows, responses
and records, mono - and its features follow the contract line by line: int64 matrix products for Re and Im, Python integers for P, E
and trunc24.  Nothing here calls the library.  The files are tests/dense_fir.py's and one more, a level-0 stream whose every sample is
-32768, which drives the DFT's sums, A and Bv to their bounds."""
import math

import numpy as np

import dense_crops as DC
import dense_fir as DF
import dense_overlay as DO
from helpers import crafted_stream
from test_block_index import expected_window

RATE = DO.RATE
FRAMES = (37, 64, 2100, 6151)
CENTER, TIME_MAJOR = 1, 2
WINDOW_MAX, CS_ONE, W_ONE = 32639, 16384, 32768
TILE = 16                               # frames of a workgroup


# ---------------------------------------------------------------------------------------------------------------- the contract

class Bank:
    """acm_feat_bank: integers as the call takes them"""

    def __init__(self, name, n_fft, hop, flags, window, cs, mel_first, mel_count, mel_off, mel_w):
        self.name, self.n_fft, self.hop, self.flags = name, n_fft, hop, flags
        self.n = n_fft.bit_length() - 1
        self.window, self.cs = np.asarray(window, np.int16), np.asarray(cs, np.int16)
        self.mel_first, self.mel_count = np.asarray(mel_first, np.uint16), np.asarray(mel_count, np.uint16)
        self.mel_off, self.mel_w = np.asarray(mel_off, np.uint32), np.asarray(mel_w, np.uint16)
        self.n_mels = self.mel_first.size
        self.center, self.time_major = bool(flags & CENTER), bool(flags & TIME_MAJOR)
        self.record = (n_fft, hop, self.n_mels, flags, self.window, self.cs, self.mel_first, self.mel_count, self.mel_off, self.mel_w)

    def frames(self, T):
        return frames(T, self.n_fft, self.hop, self.center)

    def weights(self, b):
        """(first bin, the weights) of band b"""
        first, count, off = int(self.mel_first[b]), int(self.mel_count[b]), int(self.mel_off[b])
        return first, self.mel_w[off:off + count].astype(np.int64)


def frames(T, N, H, center):
    if center:
        return 1 + T // H
    return 1 + (T - N) // H if T >= N else 0


def split(v):
    """v = 256 hi + lo, lo the signed low byte -> (hi, lo), int64"""
    v = np.asarray(v, dtype=np.int64)
    lo = ((v & 0xFF) ^ 0x80) - 0x80
    return (v - lo) >> 8, lo


def windowed(x, bank):
    """xw int64 [F, N]: the frames of row x, zeros outside [0, T), windowed"""
    N, H, T = bank.n_fft, bank.hop, x.size
    F = bank.frames(T)
    pad = N // 2 if bank.center else 0
    ext = np.zeros(pad + max(T, (F - 1) * H + N) + N, dtype=np.int64)
    ext[pad:pad + T] = x
    at = (np.arange(F) * H)[:, None] + np.arange(N)[None, :]          # place s + t + pad of ext
    return (ext[at] * bank.window.astype(np.int64)[None, :] + 16384) >> 15


def twiddles(bank):
    """(C, S) int64 [N/2 + 1, N]: c[(k t) mod N] and c[(k t + 3 N / 4) mod N]"""
    N = bank.n_fft
    kt = np.arange(N // 2 + 1)[:, None] * np.arange(N)[None, :]
    c = bank.cs.astype(np.int64)
    return c[kt % N], c[(kt + 3 * N // 4) % N]


def trunc24(E, n):
    """the float32 of include/acm_hip.h from the Python integer E"""
    if E == 0:
        return np.float32(0.0)
    p = E.bit_length() - 1
    if p > 23:
        E = (E >> (p - 23)) << (p - 23)
    return np.float32(math.ldexp(E, -(75 - 2 * n)))


def features(x, bank, detail=None):
    """float32 [B, F] of the int16 row x; detail: a dict that receives xw, A, Bv (int64) and E (Python integers [B][F])"""
    n, B = bank.n, bank.n_mels
    xw = windowed(x, bank)
    F = xw.shape[0]
    C, S = twiddles(bank)
    re, im = xw @ C.T, -(xw @ S.T)                                      # [F, N/2 + 1], exact: below 2^41
    q = n - 1
    A, Bv = (re + (1 << (q - 1))) >> q, (im + (1 << (q - 1))) >> q
    P = A.astype(object) ** 2 + Bv.astype(object) ** 2
    out = np.zeros((B, F), dtype=np.float32)
    E_all = []
    for b in range(B):
        first, w = bank.weights(b)
        E = [int(sum(int(wk) * pk for wk, pk in zip(w, P[f, first:first + w.size]))) for f in range(F)]
        out[b] = [trunc24(e, n) for e in E]
        E_all.append(E)
    if detail is not None:
        detail.update(xw=xw, A=A, Bv=Bv, E=E_all)
    return out


# ---------------------------------------------------------------------------------------------------------------- the design

def design(name, rate, n_fft=512, win_length=None, hop=160, n_mels=80, f_min=0.0, f_max=None, flags=CENTER):
    """acm_feat_design restated: periodic Hann centred in n_fft, the cosines, HTK triangles without area normalisation"""
    win_length = n_fft if win_length is None else win_length
    f_max = rate / 2.0 if f_max is None else f_max
    window = np.zeros(n_fft, np.int64)
    at = (n_fft - win_length) // 2
    window[at:at + win_length] = np.rint(WINDOW_MAX * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win_length) / win_length)))
    cs = np.rint(CS_ONE * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)).astype(np.int64)
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    corner = 700.0 * (np.power(10.0, (mel(f_min) + (mel(f_max) - mel(f_min)) * np.arange(n_mels + 2) / (n_mels + 1)) / 2595.0) - 1.0)
    fk = np.arange(n_fft // 2 + 1) * float(rate) / n_fft
    first, count, off, ws = [], [], [], []
    for b in range(n_mels):
        up, down = (fk - corner[b]) / (corner[b + 1] - corner[b]), (corner[b + 2] - fk) / (corner[b + 2] - corner[b + 1])
        q = np.rint(W_ONE * np.maximum(0.0, np.minimum(up, down))).astype(np.int64)
        nz = np.flatnonzero(q)
        lo, n = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if nz.size else (0, 0)
        first.append(lo)
        count.append(n)
        off.append(sum(w.size for w in ws))
        ws.append(q[lo:lo + n])
    return Bank(name, n_fft, hop, flags, window, cs, first, count, off, np.concatenate(ws) if ws else np.zeros(0, np.int64))


def raw_bound(name, n_fft, hop, flags, sign):
    """the bank that reaches the bounds: the window 32639 throughout, c[] = sign * 16384 throughout; band 0 of count 0, band 1 over all
    N / 2 + 1 bins with weight 32768, band 2 the single bin N / 2, band 3 a ramp over the first 16 bins - their weights share storage"""
    bins = n_fft // 2 + 1
    w = np.concatenate([np.full(bins, W_ONE), np.arange(16) * 2048 + 1])
    return Bank(name, n_fft, hop, flags, np.full(n_fft, WINDOW_MAX), np.full(n_fft, sign * CS_ONE), [5, 0, n_fft // 2, 0], [0, bins, 1, 16],
                [7, 0, bins - 1, bins], w)


# ---------------------------------------------------------------------------------------------------------------- the files

FLOOR_FILE = DF.LOUD_FILE + 1
_files = None


def files():
    """tests/dense_fir.py's, and behind them a mono level-0 stream at the batch's rate: index -1 times a header value of 32768 in every
    place - every sample is -32768"""
    global _files
    if _files is None:
        rows, nblocks = 256, 26
        floor = crafted_stream(0, rows, [(2, 32768, 3, np.full((rows, 1), -1))] * nblocks, rate=RATE)
        _files = list(DF.files()) + [DC.File(floor)]
        f = _files[FLOOR_FILE]
        assert f.channels == 1 and f.info.rate == RATE and f.words >= max(FRAMES) and (f.pcm == -32768).all()
    return _files


def index():
    return DC.index_of(files())


def data():
    return [f.data for f in files()]


# ---------------------------------------------------------------------------------------------------------------- the cases

FLOOR = DF.DRY + 1                      # the window of the floor file, behind tests/dense_fir.py's


class Case(DF.Case):
    """a mono DF.Case with one window more, FLOOR, a choice of its records (plus the identity of FLOOR) and a bank"""

    def __init__(self, base, bank, records):
        T = base.frames
        windows = [w + (sp,) for w, sp in zip(base.windows, base.speeds)] + [(FLOOR_FILE, 0, T, None)]
        super().__init__(1, T, False, windows, records, base.responses, base.of_window + [None])
        self.base, self.bank = base, bank
        self.name = "t%d_%s" % (T, bank.name)
        self.F = bank.frames(T)
        self._feats = self._detail = None

    def sources(self):
        if self._sources is None:
            floor = np.full((1, self.frames), -32768, np.int16)
            src = np.concatenate([self.base.sources(), floor])
            src.setflags(write=False)
            self._sources = src
        return self._sources

    def expect(self, k):
        f, first, count = self.windows[k]
        if f == FLOOR_FILE:
            return expected_window(files()[f].st, files()[f].rc, first, count)[:2]
        return self.base.expect(k)

    def features(self):
        """(float32 [nrows, B, F] - [nrows, F, B] for a time-major bank -, [detail per row]); computed once"""
        if self._feats is None:
            rows = self.rows()[0]
            self._detail = [{} for _ in rows]
            out = np.stack([features(row, self.bank, d) for row, d in zip(rows, self._detail)]) if len(rows) else np.zeros((0, self.bank.n_mels, self.F), np.float32)
            if self.bank.time_major:
                out = np.ascontiguousarray(out.transpose(0, 2, 1))
            out.setflags(write=False)
            self._feats = out
        return self._feats, self._detail


def ident(k):
    return (k, None, 4096, 0, 0)


_cases = None


def cases():
    """every T of FRAMES under banks that reach n_fft 128, 512 and 2048 (two K steps and more), hops 1, 37, 160 and n_fft, both
    framings, 1, 16, 17 and 33 frames - the edges of the frame tile -, 0 frames, 1, 23, 80 and 128 bands and both layouts; and the raw
    banks at the bounds.  The larger the transform, the fewer rows: the model multiplies int64 matrices"""
    global _cases
    if _cases is None:
        base = {c.frames: c for c in DF.cases() if c.channels == 1 and c.frames in FRAMES}
        D = design
        loud = [ident(FLOOR), ident(DF.LOUD), ident(DF.BEHIND), ident(DF.SPEECH), (DF.LOUD, None, 65535, 0, 0)]
        some = [(DF.SPEECH, DF.UP, 4096, DO.SNR10, 0), (DF.LOUD, DF.UP, 4096, DO.SNR10, 0), (DF.CUT, DF.SHORT, 4096, 0, 32768), ident(DF.SPEECH),
                ident(DF.BEHIND), ident(DF.LOUD30), ident(FLOOR), (DF.WIDE, DF.DRY, 4096, DO.SNR10, 0)]
        every = lambda T: base[T].records + [ident(FLOOR)]
        plan = [
            (37, D("d512_h160_b80", 16000), some),                                                                                # F 1
            (37, D("d128_hN_b23_whole_tm", 16000, 128, None, 128, 23, flags=TIME_MAJOR), some),                                   # T < N: F 0
            (37, D("d512_h37_b80_tm", 16000, 512, None, 37, 80, flags=CENTER | TIME_MAJOR), some),                                # F 2
            (64, D("d128_h1_b23", 16000, 128, None, 1, 23, 100.0, 7000.0), every(64)),                                            # hop 1: F 65
            (64, raw_bound("raw128_plus", 128, 64, CENTER, 1), loud),                                                             # every frame half outside
            (2100, raw_bound("raw128_plus", 128, 128, CENTER, 1), loud),                                                          # frames 1 .. 15 inside the row
            (2100, raw_bound("raw128_minus_tm", 128, 37, CENTER | TIME_MAJOR, -1), loud),
            (2100, D("d512_h160_b80", 16000), every(2100)),                                                                       # the README's bank: F 14
            (2100, D("d512_w400_h160_b80_tm", 16000, 512, 400, 160, 80, flags=CENTER | TIME_MAJOR), some),
            (2100, D("d128_hN_b23_whole_tm", 16000, 128, None, 128, 23, flags=TIME_MAJOR), some),                                 # F 16
            (2100, D("d128_hN_b23", 16000, 128, None, 128, 23), some),                                                            # F 17
            (2100, D("d2048_h160_b1_whole", 16000, 2048, None, 160, 1, flags=0), some[:3]),                                       # F 1
            (2100, raw_bound("raw2048_plus_whole", 2048, 2048, 0, 1), loud[:2]),                                                  # one whole frame: the partial sums at N 2048
            (6151, D("d2048_h192_b128_tm", 16000, 2048, None, 192, 128, flags=CENTER | TIME_MAJOR), some[:2]),                    # F 33
            (6151, D("d512_h160_b80", 16000), some),                                                                              # F 39
            (6151, D("d128_h37_b128_whole", 16000, 128, None, 37, 128, flags=0), some[:3]),                                       # F 163
        ]
        _cases = [Case(base[T], bank, records) for T, bank, records in plan]
    return _cases
