"""The model and the cases of log-mel features from dense crop batches (acm_batch_decode_windows_logmel, include/acm_hip.h), for
tests/test_dense_logmel.py (the integer logarithm, the scale, the check, the cases' own coverage, without a GPU) and
tests/test_gpu_dense_logmel.py (the call itself).

The call continues acm_batch_decode_windows_features' contract behind its mel sum E, so the model continues tests/dense_feat.py's:
E as Python integers from Case.features(), then the contract's lines - mantissa, fraction, L, floor, top, scale - on integers (the
sixteen squarings vectorised over uint64, where a square stays below 2^48).  Nothing here calls the library.

The cases are the smallest of tests/dense_feat.py's, each under four scales, and three of this module's own with quiet rows: a volume of
1 / 4096 and 2 / 4096 leaves samples of a few units, whose energies lie around the floor of 1e-10."""
import numpy as np

import dense_feat as M
import dense_fir as DF

TOP = 1                                 # ACM_FEAT_LOG_TOP
FLOOR_MAX, MUL_MAX, TOP_MAX = 64 * 65536, 1 << 28, 128 * 65536


# ---------------------------------------------------------------------------------------------------------------- the contract

class Scale:
    """acm_feat_log: integers as the call takes them"""

    def __init__(self, name, flags, floor_q16, mul_q24, offset_q16, top_q16):
        self.name, self.flags, self.floor_q16, self.mul_q24, self.offset_q16, self.top_q16 = name, flags, floor_q16, mul_q24, offset_q16, top_q16
        self.top = bool(flags & TOP)
        self.record = (flags, floor_q16, mul_q24, offset_q16, top_q16)


# the four scales every case runs under, their fields worked out by hand:
#   log2(1e-10) = -33.21928094887362 -> floor_q16 -2177059;  2^24 ln 2 = 11629079.9, 2^24 log10 2 = 5050445.3 (a quarter: 1262611.3),
#   2^24 * 10 log10 2 = 50504452.6;  80 / (10 log10 2) = 8 / log10 2 = 26.5754247591 -> top_q16 1741647
LOG2 = Scale("log2", 0, -FLOOR_MAX, 1 << 24, 0, 0)
LN = Scale("ln", 0, -2177059, 11629080, 0, 0)
DB80 = Scale("db_top80", TOP, -2177059, 50504453, 0, 1741647)
WHISPER = Scale("whisper", TOP, -2177059, 1262611, 65536, 1741647)
SCALES = (LOG2, LN, DB80, WHISPER)
# ... and a narrow top for the quiet cases, 30 dB, with a scale and an offset that are no round numbers
DB30 = Scale("db_top30", TOP, -2177059, 50504453, -12345, 653118)


def frac(m):
    """frac of include/acm_hip.h, of an array of mantissas in [2^23, 2^24) -> (uint64 array of the sixteen bits, whether x stayed in
    [2^23, 2^24) throughout)"""
    x = np.asarray(m, dtype=np.uint64)
    f = np.zeros(x.shape, dtype=np.uint64)
    inside = True
    for _ in range(16):
        x = x * x
        bit = (x >= np.uint64(1 << 47)).astype(np.uint64)
        x = x >> (np.uint64(23) + bit)
        f = (f << np.uint64(1)) | bit
        inside = inside and bool(((x >= np.uint64(1 << 23)) & (x < np.uint64(1 << 24))).all())
    return f, inside


def lead(E):
    """(p, m) of the Python integer E >= 1: the position of its leading bit and its 24 leading bits"""
    p = E.bit_length() - 1
    return p, (E >> (p - 23) if p > 23 else E << (23 - p))


def log_q16(E, n, floor_q16):
    """L of an array-like of Python integers E -> int64 array of the same shape"""
    flat = [int(e) for e in np.asarray(E, dtype=object).reshape(-1)]
    live = np.array([e > 0 for e in flat], dtype=bool)
    pm = [lead(e) for e in flat if e > 0]
    L = np.full(len(flat), floor_q16, dtype=np.int64)
    if pm:
        p = np.array([v[0] for v in pm], dtype=np.int64)
        f = frac(np.array([v[1] for v in pm], dtype=np.uint64))[0].astype(np.int64)
        L[live] = (p - (75 - 2 * n)) * 65536 + f
    return np.maximum(L, floor_q16).reshape(np.asarray(E, dtype=object).shape)


def scaled(L, scale):
    """V of L (int64 array)"""
    return ((L.astype(np.int64) * scale.mul_q24 + (1 << 23)) >> 24) + scale.offset_q16


def row_logmel(E, n, scale, detail=None):
    """float32 [B, F] of one row's E ([B][F] Python integers); detail receives L (before the top), M_r, the clamped L and V"""
    L = log_q16(E, n, scale.floor_q16)
    top = int(L.max()) if L.size else scale.floor_q16
    Lc = np.maximum(L, top - scale.top_q16) if scale.top else L
    V = scaled(Lc, scale)
    assert not V.size or np.abs(V).max() < 1 << 24
    if detail is not None:
        detail.update(L=L, M=top, Lc=Lc, V=V)
    return (V.astype(np.float64) / 65536.0).astype(np.float32)


def check(scale_record, reserved=0):
    """acm_feat_log_check's own part restated: True for a scale the call takes"""
    flags, floor_q16, mul_q24, offset_q16, top_q16 = scale_record
    if flags & ~TOP or reserved or not -FLOOR_MAX <= floor_q16 <= FLOOR_MAX or not 1 <= mul_q24 <= MUL_MAX or not 0 <= top_q16 <= TOP_MAX:
        return False
    if top_q16 and not flags & TOP:
        return False
    Lb = max(62 * 65536, abs(floor_q16))
    return ((Lb * mul_q24) >> 24) + abs(offset_q16) + 1 < 1 << 24


# ---------------------------------------------------------------------------------------------------------------- the cases

class LogCase:
    """a tests/dense_feat.py Case under a Scale"""

    def __init__(self, case, scale):
        self.case, self.scale = case, scale
        self.name = "%s_%s" % (case.name, scale.name)
        self._out = self._detail = None

    def logmel(self):
        """(float32 [nrows, B, F] - [nrows, F, B] for a time-major bank -, [detail per row]); computed once"""
        if self._out is None:
            c = self.case
            E = c.features()[1]
            self._detail = [{} for _ in E]
            rows = [row_logmel(np.array(d["E"], dtype=object).reshape(c.bank.n_mels, c.F), c.bank.n, self.scale, out) for d, out in zip(E, self._detail)]
            out = np.stack(rows) if rows else np.zeros((0, c.bank.n_mels, c.F), np.float32)
            if c.bank.time_major:
                out = np.ascontiguousarray(out.transpose(0, 2, 1))
            out.setflags(write=False)
            self._out = out
        return self._out, self._detail


BASE = ("t37_d512_h37_b80_tm", "t64_raw128_plus", "t2100_d128_hN_b23", "t2100_d512_h160_b80", "t6151_d128_h37_b128_whole")
_own = _cases = None


def quiet(k, vol):
    """window k at a volume of vol / 4096: samples of a few units"""
    return (k, None, vol, 0, 0)


def own():
    """this module's Cases by name: `loud` and `quiet` share a bank and a row count (tests/test_gpu_dense_logmel.py runs them in turn
    on one handle), `tail` has 163 frames, eleven tiles, of rows that are loudest at their end"""
    global _own
    if _own is None:
        base = {c.frames: c for c in DF.cases() if c.channels == 1 and c.frames in M.FRAMES}
        D = M.design
        small = D("d128_hN_b23", 16000, 128, None, 128, 23)
        wide = D("d128_h37_b128_whole", 16000, 128, None, 37, 128, flags=0)
        _own = {"loud": M.Case(base[2100], small, [M.ident(DF.LOUD), M.ident(M.FLOOR), M.ident(DF.SPEECH)]),
                "quiet": M.Case(base[2100], small, [quiet(DF.SPEECH, 1), M.ident(DF.BEHIND), quiet(DF.LOUD, 2)]),
                "tail": M.Case(base[6151], wide, [quiet(DF.SPEECH, 1), M.ident(DF.SPEECH), quiet(DF.WIDE, 3)])}
        for name, c in _own.items():
            c.name = "%s_%s" % (name, c.name)
    return _own


def feat_case(name):
    return next(c for c in M.cases() if c.name == name)


def cases():
    """the five smallest cases of tests/dense_feat.py under the four scales, and this module's own under the scales with a top"""
    global _cases
    if _cases is None:
        _cases = [LogCase(feat_case(name), s) for name in BASE for s in SCALES]
        _cases += [LogCase(c, s) for c in own().values() for s in (DB30, WHISPER)] + [LogCase(own()["quiet"], LN)]
    return _cases


def pick(name):
    return next(c for c in cases() if c.name == name)
