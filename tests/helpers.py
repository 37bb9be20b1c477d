"""Shared test helpers: synthetic streams + the oracle's answer for them."""
import numpy as np

import oracle_api as O
from libacm_amd import capi, synth


# The GPU tests never compare against memory a previous call wrote: every module of them imports this one, and with the switch on the capi
# helpers turn the fill mode of whatever device handle they are given on (acmhip_device_set_fill: reused staging arenas and recycled plan
# blocks start each call filled) and capi.synth poisons its PCM buffer.  bench.py and the measurement scripts under profiles/ do not
# import this module (the fuzzers there do: they are checks like these)
capi.FILL_MODE = True


def poison_pcm(dev, d_pcm, words, f32=False):
    """what a test that launches a plan into a PCM buffer of its own does before EVERY launch: 0xA5 bytes under `words` 16-bit samples,
    0xFF bytes under `words` floats (capi.POISON16 / POISON32 per word) - a sample no kernel wrote is then not the previous launch's"""
    dev.memset(d_pcm, 0xFF if f32 else 0xA5, words * (4 if f32 else 2))


def make_stream(seed, level, rows, nblocks, channels=1, cut=0, **kw):
    """One synthetic file; `cut` trims total_values so it is not block aligned."""
    total = max(1, nblocks * rows * (1 << level) - cut)
    return synth.generate(seed=synth.BASE_SEED + seed, level=level, rows=rows, nblocks=nblocks,
                          channels=channels, total_values=total, **kw)


def plan_rows(level):
    """rows the planner hands out at a time: whole tiles of the lean kernel's vector-ALU build, cut into the byte-plane build's own (a level
    of the chunk kernel: 2048-sample chunks; level 13: row pairs)"""
    return max(capi.lib().acmhip_mform_tile_rows(level), capi.lib().acmk_tile2_rows(level), 4)


def oracle_pcm(data, force_chans=0, be=0, sgned=1):
    """Whole-file decode by the CPU oracle -> (uint16 view of the output bytes, status)."""
    pcm, st = O.Oracle.decode_all(data, force_chans=force_chans, be=be, sgned=sgned)
    return pcm.view(np.uint16), st


def fmt_args(fmt):
    """ACMHIP_FMT_* -> (bigendianp, sgned)"""
    return (fmt & 1), (0 if fmt & 2 else 1)


def juggle_inputs(level, rows, nblocks=4):
    """Deterministic raw int32 block matrices for the juggle_block vectors (golden family F9):
    full-range values, except block 1 which has realistic magnitudes."""
    rng = np.random.default_rng([0xAC3D, level, rows])
    cols = 1 << level
    out = []
    for b in range(nblocks):
        blk = rng.integers(-2 ** 31, 2 ** 31 - 1, size=rows * cols, dtype=np.int64).astype(np.int32)
        if b == 1:
            blk = (blk >> 14).astype(np.int32)
        out.append(blk)
    return out


import hashlib
import json
import os

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_golden = None


def golden():
    global _golden
    if _golden is None:
        with open(os.path.join(GOLDEN_DIR, "golden.json")) as f:
            _golden = json.load(f)["cases"]
    return _golden


def golden_file(name):
    with open(os.path.join(GOLDEN_DIR, "acm", name + ".acm"), "rb") as f:
        return f.read()


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


REF_ANSWERS = os.path.join(GOLDEN_DIR, "ref_answers.json")
RECORDING = None            # a dict while tests/golden/make_golden_ref_answers.py records the live reference's answers into it
_ref_answers = None


class RefAnswers:
    """The compiled reference's answers to one test's sequence of questions, in order.  Replayed from tests/golden/ref_answers.json,
    so the test needs nothing outside the repository; tests/golden/make_golden_ref_answers.py runs the same tests against the live
    reference (oracle/_ref) to record them.  ask(fn): fn() questions the live reference and returns a JSON value (digests in place
    of PCM bytes); it is only called while recording."""

    def __init__(self, key):
        global _ref_answers
        self.key, self.i = key, 0
        self.live = RECORDING is not None
        if self.live:
            self.vals = RECORDING[key] = []
        else:
            if _ref_answers is None:
                with open(REF_ANSWERS) as f:
                    _ref_answers = json.load(f)
            self.vals = _ref_answers[key]

    def ask(self, fn):
        if self.live:
            self.vals.append(json.loads(json.dumps(fn())))
        assert self.i < len(self.vals), "%s: more questions than recorded answers" % self.key
        self.i += 1
        return self.vals[self.i - 1]

    def done(self):
        assert self.i == len(self.vals), "%s: %d of %d recorded answers asked for" % (self.key, self.i, len(self.vals))


def decode_record(stream_cls_factory, data, force_chans=0, be=0, sgned=1, step=8192, **io_kw):
    """Decode through any libacm.h-shaped stream wrapper and summarise like make_golden.ref_decode()."""
    s = stream_cls_factory(data, force_chans, **io_kw)
    if s.err < 0:
        return {"open": s.err}
    pcm, rc = s.decode_all(step, be, sgned)
    rec = {"open": 0, "status": rc, "words": len(pcm) // 2, "sha256": sha(pcm),
           "head": [int(x) for x in np.frombuffer(pcm[:128], dtype="<u2")],
           "tail": [int(x) for x in np.frombuffer(pcm[-128:], dtype="<u2")] if len(pcm) >= 128 else [],
           "info": s.info(), "raw_tell_end": s.getter("raw_tell")}
    s.close()
    return rec


class BitWriter:
    """Bits LSB first, as libacm_amd/csrc/acm_synth.c writes them: fields are kept as arrays of single bits and packed once (numpy
    unpackbits / packbits), so a stream of a few hundred thousand fields costs milliseconds."""

    def __init__(self):
        self.parts = []

    def put(self, v, n):
        self.put_many([int(v) & ((1 << n) - 1)], n)

    def put_many(self, values, n):
        """every value of `values` as an n-bit field (n <= 16), one behind the other"""
        if n:
            v = np.ascontiguousarray(values, dtype="<u2").reshape(-1, 1)
            self.parts.append(np.unpackbits(v.view(np.uint8), axis=1, bitorder="little")[:, :n].reshape(-1))

    def put_bits(self, bits):
        self.parts.append(np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1))

    def stream_header(self, level, rows, total, channels, rate):
        """reader: decode.c:712-752"""
        for v, n in ((0x97, 8), (0x28, 8), (0x03, 8), (1, 8), (total & 0xFFFF, 16), (total >> 16, 16), (channels, 16), (rate, 16), (level, 4), (rows, 12)):
            self.put(v, n)

    def bytes(self):
        """the stream so far, its last byte filled up with zero bits"""
        return np.packbits(np.concatenate(self.parts) if self.parts else np.zeros(0, np.uint8), bitorder="little").tobytes()


def handmade_stream(level, rows, blocks, channels=1, rate=22050, seed=1):
    """An ACM file written by hand (bits LSB first, as libacm_amd/csrc/acm_synth.c writes them; reader: decode.c:586-589 block
    header, :491-502 column loop, :712-752 stream header): `blocks` = [(pwr, val, code)], every column of a block uses the one
    filler `code` - 0 (no payload) or a linear width 3..16 (rows x code bits, random; keep code <= pwr + 1).  For files whose
    bit rate is as uneven as one likes (the striped upload of acm_batch.cpp has to notice)."""
    rng = np.random.default_rng([0xACE5, seed, level, rows])
    w = BitWriter()
    cols = 1 << level
    w.stream_header(level, rows, len(blocks) * rows * cols, channels, rate)
    for pwr, val, code in blocks:
        assert code == 0 or 3 <= code <= min(16, pwr + 1)
        w.put(pwr, 4)
        w.put(val, 16)
        for _ in range(cols):
            w.put(code, 5)
            if code:
                w.put_many(rng.integers(0, 1 << code, size=rows), code)
    return w.bytes()


def crafted_stream(level, rows, blocks, channels=1, cut=0, rate=22050):
    """An ACM file with CHOSEN indices, header and bit order as handmade_stream writes them: `blocks` = [(pwr, val, code, idx)], idx an int
    array of shape (rows, 1 << level), `code` one linear filler width 3..16 for the whole block (filler value = idx + 2^(code-1)).  Every
    index lies inside the filler's range and code <= pwr + 1, so every index is inside the block's own amplitude table: no H1 patch.
    `cut` trims total_values so that the stream does not end on a block boundary."""
    w = BitWriter()
    cols = 1 << level
    w.stream_header(level, rows, max(1, len(blocks) * rows * cols - cut), channels, rate)
    for pwr, val, code, idx in blocks:
        idx = np.asarray(idx)
        assert idx.shape == (rows, cols) and 3 <= code <= min(16, pwr + 1) and 0 <= pwr <= 15 and 0 <= val <= 65535
        half = 1 << (code - 1)
        assert -half <= int(idx.min()) and int(idx.max()) < half, (code, int(idx.min()), int(idx.max()))
        w.put(pwr, 4)
        w.put(val, 16)
        # column by column: the 5-bit code, then the column's `rows` values of `code` bits each
        fill = np.ascontiguousarray((idx.T.astype(np.int64) + half).astype("<u2")).reshape(cols, rows, 1)
        bits = np.empty((cols, 5 + rows * code), dtype=np.uint8)
        bits[:, :5] = (code >> np.arange(5)) & 1
        bits[:, 5:] = np.unpackbits(fill.view(np.uint8), axis=2, bitorder="little")[:, :, :code].reshape(cols, rows * code)
        w.put_bits(bits)
    return w.bytes()
