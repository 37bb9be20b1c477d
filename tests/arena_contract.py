"""Arenas that use everything include/acm_hip.h allows a stream descriptor, for tests/test_arena_contract.py (host synthesis, no GPU) and
tests/test_gpu_arena_contract.py (every kernel family).

The header promises: idx_off and pcm_off are multiples of 8 words (not of 64, which is what capi.Arena, the workload builders and the
other tests hand out), hdr_off is any header index, and n_emit is "samples to write" - not one word more is written.  contract(level)
lays out, for one level:

  * sources: two whole files (make_stream(..., cut=0): the oracle's PCM covers every staged row) of block height 3 and 16 (1 and 2 at
    levels 13-15), and at levels 3, 6 and 9 a third one with H1 patches.  R staged rows each, the fewest whole blocks with
    R >= 2 T + 3 and R * cols >= 2048, T the level's largest tile height (tile_height): a whole lean tile, a second one, a ragged rest;
  * the index arena: four copies of every source, at every residue of 8 words modulo 64 (A: 8, 24, 40, 56; B: 0, 16, 32, 48; C: non-zero
    ones), at least 8 words of index 0x7FFF in front of, between and behind them - a kernel that reads beyond a stream's staged rows and
    lets it reach a sample computes a wrong one;
  * the header arena: the copies' header runs with one to three poison headers (val 0xFFFF, pwr 15) in front of each: hdr_off is odd
    and even and never 0;
  * descriptors, round-robin over a source's copies: from row 0 with n_emit around a row, a tile, two tiles and the last eight counts up
    to the whole stream (every n_emit mod 8); windows from rows 1, 2, T and T + 1 that end 0, 3 and 5 samples short of the stream, and
    of 11 samples;
  * the PCM arena: slot k on the first multiple of 8 that leaves 8 words behind the slot in front of it and is 8 (k mod 8) modulo 64,
    64 words behind the last one.  Everything outside [pcm_off, pcm_off + n_emit) of the slots must keep the poison it is filled with
    before a launch: `mask`.

Expected PCM is the oracle's whole decode of the source (tests/oracle_api.py), sliced."""
import ctypes as C
import functools

import numpy as np

from helpers import fmt_args, make_stream, oracle_pcm
from libacm_amd import capi

IDX_POISON = 0x7FFF
HDR_POISON = (0xFFFF, 15)
POISON16, POISON32 = 0xA5A5, 0xFFFFFFFF         # the PCM arena before a launch: 0xA5 bytes (int16), 0xFF bytes (float32: a NaN)
H1_LEVELS = (3, 6, 9)
RESIDUES = ((8, 24, 40, 56), (0, 16, 32, 48), (16, 40, 56, 8))         # idx_off mod 64 of the four copies of source A, B, C
COPIES = 4
F32 = "f32"                                     # beside capi.FMT_*: the float32 launch
FORMATS = (capi.FMT_S16LE, capi.FMT_S16BE, capi.FMT_U16LE, capi.FMT_U16BE)


def tile_height(level):
    """the largest tile height of a level: the lean kernels' tile, else the fused tile kernel's payload rows, else 64 rows"""
    L = capi.lib()
    if L.acmk_tile2_rows(level):
        return L.acmk_tile2_rows(level)
    return L.acmk_fused_tile_rows(level, 0) - 2 if L.acmk_fused_tile_rows(level, 0) else 64


def f32_bits(u16):
    """the float32 sample of an s16le sample, as bits: the sample times 2^-15, exactly"""
    return (np.asarray(u16).view(np.int16).astype(np.float32) / np.float32(32768)).view(np.uint32)


class Source:
    def __init__(self, name, data, staged):
        self.name, self.data, self.st = name, data, staged
        self.rows = staged.info.rows
        self.nrows = staged.info.blocks * staged.info.rows
        self.patches = list(staged.patches) if staged.patches is not None else []
        self.idx_off, self.hdr_off = [], []             # of its copies
        self._pcm = {}

    def pcm(self, fmt):
        """the oracle's whole decode in format fmt (uint16 view; F32: the float bits)"""
        if fmt not in self._pcm:
            if fmt == F32:
                self._pcm[fmt] = f32_bits(self.pcm(capi.FMT_S16LE))
            else:
                be, sg = fmt_args(fmt)
                self._pcm[fmt] = oracle_pcm(self.data, 0, be, sg)[0]
                assert self._pcm[fmt].size == self.nrows << self.st.info.level        # a whole file: every staged row
        return self._pcm[fmt]


def _h1_source(level, rows, nblocks):
    for seed in range(40):
        f = make_stream(31500 + 64 * level + seed, level, rows, nblocks, mix=1, allow_out_of_range=1, prime_table=1, pwr_min=0, pwr_max=6)
        s = capi.stage_file(f)
        if s.patches is not None and len(s.patches):
            return f, s
    raise AssertionError("no H1-patched stream of level %d found" % level)


def emit_counts(cols, T, R):
    """n_emit of the descriptors that start at row 0"""
    want = [1, 5, 8, 13, cols - 1, cols, cols + 3, T * cols - 1, T * cols, T * cols + 1, T * cols + 9, 2 * T * cols - 7]
    want += [R * cols - k for k in range(8)]
    out = []
    for v in want:
        if 1 <= v <= R * cols and v not in out:
            out.append(v)
    return out


def window_shapes(cols, T, R):
    """(row_begin, n_emit) of the windows"""
    out = []
    for rb in (1, 2, T, T + 1):
        for v in [(R - rb) * cols - k for k in (0, 3, 5)] + [11]:
            if 1 <= v <= (R - rb) * cols and (rb, v) not in out:
                out.append((rb, v))
    return out


def _next_at(at, gap, residue):
    """the first multiple of 8 that is >= at + gap and is `residue` modulo 64"""
    p = (at + gap + 7) & ~7
    return p + (residue - p) % 64


class Contract:
    """one level's arenas: .sources, .descs (+ .desc_source / .desc_copy: which copy of which source a descriptor reads), .patches (a
    ctypes array over all descriptors, or None), .idx, .hdr, .pcm_words, .mask; expected(fmt) / expected_arena(fmt) / poisoned(fmt)"""

    def __init__(self, level):
        self.level, self.cols, self.T = level, 1 << level, tile_height(level)
        cols, T = self.cols, self.T
        need = max(2 * T + 3, (2048 + cols - 1) // cols)
        heights = (1, 2) if level >= 13 else (3, 16)
        self.sources = []
        for k, rows in enumerate(heights):
            nb = (need + rows - 1) // rows
            f = make_stream(31000 + 16 * level + k, level, rows, nb, cut=0, channels=1 + k % 2 if cols > 1 else 1)
            self.sources.append(Source("AB"[k], f, capi.stage_file(f)))
        if level in H1_LEVELS:
            f, s = _h1_source(level, 4, (need + 3) // 4)
            self.sources.append(Source("C", f, s))
        for s in self.sources:
            assert s.st.info.end_status == 0 and s.st.words == s.nrows * cols and s.nrows >= need, (level, s.name)

        # index and header arenas: the copies of A, B (, C) in turn
        lay, at, hat = [], 0, 0
        for c in range(COPIES):
            for k, s in enumerate(self.sources):
                at = _next_at(at, 8, RESIDUES[k][c])
                gap = 1 + len(lay) % 3                  # one to three poison headers; odd and even hdr_off take turns
                if (hat + gap) % 2 != len(lay) % 2:
                    gap += 1 if gap < 3 else -1
                hat += gap
                lay.append((s, at, hat))
                s.idx_off.append(at)
                s.hdr_off.append(hat)
                at += s.nrows * cols
                hat += s.st.info.blocks
        self.idx = np.full(at + 64, IDX_POISON, dtype=np.int16)
        self.hdr = np.empty((hat + 3, 2), dtype=np.uint32)
        self.hdr[:] = HDR_POISON
        self.staged_words = np.zeros(self.idx.size, dtype=bool)
        for s, io, ho in lay:
            self.idx[io:io + s.nrows * cols] = s.st.idx[:s.nrows * cols]
            self.hdr[ho:ho + s.st.info.blocks] = s.st.hdr[:s.st.info.blocks]
            self.staged_words[io:io + s.nrows * cols] = True

        # descriptors and the PCM arena
        self.descs, self.desc_source, self.desc_copy, plist = [], [], [], []
        end = 0
        for k, s in enumerate(self.sources):
            R = s.nrows
            shapes = [(0, v) for v in emit_counts(cols, T, R)] + window_shapes(cols, T, R)
            for j, (rb, ne) in enumerate(shapes):
                i = len(self.descs)
                c = j % COPIES
                po = _next_at(end, 8, 8 * (i % 8))
                self.descs.append(capi.StreamDesc(idx_off=s.idx_off[c], hdr_off=s.hdr_off[c], pcm_off=po, n_emit=ne, level=level, rows=s.rows,
                                                  nrows=R, row_begin=rb))
                self.desc_source.append(k)
                self.desc_copy.append(c)
                plist += [capi.Patch(p.sample, p.value, i) for p in s.patches]
                end = po + ne
        self.pcm_words = end + 64
        self.patches = (capi.Patch * len(plist))(*plist) if plist else None
        self.mask = np.ones(self.pcm_words, dtype=bool)
        for d in self.descs:
            self.mask[d.pcm_off:d.pcm_off + d.n_emit] = False
        self._arena = {}

    def whole_copy_descs(self):
        """one descriptor per copy of every source, from row 0 over all its rows (what the second staged forms are built from), and
        per descriptor of .descs which of them it reads"""
        whole, at = [], {}
        for k, s in enumerate(self.sources):
            for c in range(COPIES):
                at[(k, c)] = len(whole)
                whole.append(capi.StreamDesc(idx_off=s.idx_off[c], hdr_off=s.hdr_off[c], pcm_off=0, n_emit=s.nrows * self.cols, level=self.level,
                                             rows=s.rows, nrows=s.nrows, row_begin=0))
        return whole, [at[(k, c)] for k, c in zip(self.desc_source, self.desc_copy)]

    def expected(self, i, fmt):
        """what descriptor i's slot holds after a launch in format fmt"""
        d = self.descs[i]
        lo = d.row_begin * self.cols
        return self.sources[self.desc_source[i]].pcm(fmt)[lo:lo + d.n_emit]

    def poisoned(self, fmt):
        return np.full(self.pcm_words, POISON32 if fmt == F32 else POISON16, dtype=np.uint32 if fmt == F32 else np.uint16)

    def expected_arena(self, fmt):
        """the whole PCM arena after a launch in format fmt into a poisoned arena (kept for the last format asked for only: level 15's
        is a few hundred megabytes)"""
        if fmt not in self._arena:
            self._arena.clear()
            a = self.poisoned(fmt)
            for i, d in enumerate(self.descs):
                a[d.pcm_off:d.pcm_off + d.n_emit] = self.expected(i, fmt)
            self._arena[fmt] = a
        return self._arena[fmt]

    def describe(self, i):
        d = self.descs[i]
        return "desc %d (level %d, source %s copy %d, idx_off %d hdr_off %d pcm_off %d, row_begin %d, n_emit %d)" % (
            i, d.level, self.sources[self.desc_source[i]].name, self.desc_copy[i], d.idx_off, d.hdr_off, d.pcm_off, d.row_begin, d.n_emit)

    def check(self, got, fmt, what=""):
        """got: the PCM arena after a launch in format fmt into poisoned(fmt).  Every slot is the oracle's slice and every other word
        keeps the poison - or an AssertionError that names the descriptor: for a dirty guard word the one in front of it and how far
        behind that descriptor's n_emit the word lies, for a wrong sample the slot's own"""
        want = self.expected_arena(fmt)
        assert got.shape == want.shape and got.dtype == want.dtype
        if np.array_equal(got, want):
            return
        bad = np.nonzero(got != want)[0]
        dirty = bad[self.mask[bad]]
        starts = np.array([d.pcm_off for d in self.descs])
        if dirty.size:
            w = int(dirty[0])
            i = int(np.searchsorted(starts, w, side="right")) - 1
            if i < 0:
                raise AssertionError("%s format %s: %d guard words written, the first %d words in front of the first slot" % (what, fmt, dirty.size, starts[0] - w))
            d = self.descs[i]
            behind = ", %d words in front of desc %d" % (starts[i + 1] - w, i + 1) if i + 1 < len(starts) else ""
            raise AssertionError("%s format %s: %d guard words written; the first, word %d (0x%x), lies %d words behind the n_emit of %s%s"
                                 % (what, fmt, dirty.size, w, int(got[w]), w - (d.pcm_off + d.n_emit), self.describe(i), behind))
        w = int(bad[0])
        i = int(np.searchsorted(starts, w, side="right")) - 1
        raise AssertionError("%s format %s: %d samples differ from the oracle's; the first is sample %d of %s: 0x%x, expected 0x%x"
                             % (what, fmt, bad.size, w - self.descs[i].pcm_off, self.describe(i), int(got[w]), int(want[w])))


@functools.lru_cache(maxsize=2)
def contract(level):
    """the level's arenas, built once and shared (read-only) by the tests of that level"""
    return Contract(level)


def valid_desc(d):
    """acmhip_plan_create's rule for a descriptor (libacm_amd/csrc/acm_plan_cut.cpp: valid_desc)"""
    return (d.level <= 15 and 1 <= d.rows <= 4095 and d.idx_off % 8 == 0 and d.pcm_off % 8 == 0 and d.row_begin <= d.nrows and
            d.n_emit <= (d.nrows - d.row_begin) << d.level)


def host_launch(ct, fmt):
    """acmhip_host_synth / acmhip_host_synth_f32 of every descriptor on the contract arenas, with the arenas' own offsets, into one
    poisoned PCM arena -> that arena"""
    L = capi.lib()
    out = ct.poisoned(fmt)
    for i, d in enumerate(ct.descs):
        pl = ct.sources[ct.desc_source[i]].patches
        arr = (capi.Patch * len(pl))(*pl) if pl else None
        if fmt == F32:
            rc = L.acmhip_host_synth_f32(C.byref(d), ct.idx.ctypes.data, ct.hdr.ctypes.data, arr, len(pl), out.ctypes.data)
        else:
            rc = L.acmhip_host_synth(C.byref(d), ct.idx.ctypes.data, ct.hdr.ctypes.data, arr, len(pl), fmt, out.ctypes.data)
        assert rc == 0, (ct.describe(i), rc)
    return out
