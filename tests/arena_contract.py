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

Expected PCM is the oracle's whole decode of the source (tests/oracle_api.py), sliced.

far_contract(level) / far_form(level, form), at the end of this file, are the same contract at offsets past 32 bits, as pieces, for
tests/test_gpu_far_offsets.py."""
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


# ---- the far variant: the same contract at offsets past 32 bits ---------------------------------------------------------------------------

E30, E31, E32 = 1 << 30, 1 << 31, 1 << 32       # elements; E31 int16 elements (and E30 floats) are byte 2^32
H29 = 1 << 29                                   # header entries (8 bytes each): byte 2^32
FILL = 0x7F                                     # what the index and header arenas hold outside their pieces: an index is 0x7F7F
FAR_RUNS = 4


def _mod_pieces(lo, hi, m):
    """[lo, hi) modulo m, where that is not [lo, hi) itself: a list of (a, b, what was subtracted)"""
    out = []
    for k in range(max(lo // m, 1), (hi - 1) // m + 1):
        out.append((max(lo, k * m) - k * m, min(hi, (k + 1) * m) - k * m, k * m))
    return out


def _own_alias(lo, hi, src, placed, moduli, data=None):
    """how far [lo, hi) has to move up before its first alias (modulo any of moduli) that lies on a run of its own source in
    `placed` ([lo, hi, src, ...]) is clear of that run; 0: every alias of every unit lies on the fill or on another source's run.
    data ({source: its run's units}): an alias on the run's own source counts only where it would forgive - where fewer than three
    quarters of the units the alias overlaps differ from the units that belong there (the same data displaced is other data)"""
    bump = 0
    for m in moduli:
        for a, b, sub in _mod_pieces(lo, hi, m):
            for p in placed:
                if p[2] == src and a < p[1] and p[0] < b:
                    if data is not None:
                        x, y = max(a, p[0]), min(b, p[1])
                        mine, theirs = data[src][x + sub - lo:y + sub - lo], data[src][x - p[0]:y - p[0]]
                        if 4 * int(np.count_nonzero(mine != theirs if mine.ndim == 1 else (mine != theirs).any(axis=1))) >= 3 * (y - x):
                            continue
                    bump = max(bump, p[1] - a)
    return bump


def lay_far(runs, groups, step, gap, moduli, data, astride=None):
    """Lays runs out sparsely.  runs: {key: (source, length, near offset)}, key = (source, copy); groups: [(boundary, [keys])], the
    boundaries ascending; every run in no group stays at its near offset; data: {source: its units}.  Per group one run of the group's
    first copy straddles the boundary (the boundary lies strictly inside it), as near its middle as the alias rule lets it, and the others
    follow behind it, the later copies first, each at the first offset that leaves `gap` units behind the run in front, equals its near
    offset modulo `step` and keeps the alias rule: NO unit of a moved run has an alias - its offset modulo one of `moduli` - on a run of
    the same source.  Where no run can straddle under that rule (the units in front of E32 alias to the units in front of E31: with two
    sources, and source A unable to straddle, both boundaries fall to B), the straddler's aliases may lie on its own source's data
    DISPLACED: at least three quarters of the units differ from what belongs there, checked on the data.
    astride: the sources whose runs may straddle (default: any).  -> ({key: offset}, the keys placed under the weaker rule)"""
    far = [k for _, keys in groups for k in keys]
    placed = [[off, off + n, src, key] for key, (src, n, off) in runs.items() if key not in far]
    out = {key: off for key, (src, n, off) in runs.items() if key not in far}
    displaced = []
    for boundary, keys in groups:
        best = None
        for weak in (None, data):
            for key in (k for k in keys if k[1] == min(q[1] for q in keys) and (astride is None or k[0] in astride)):
                src, n, off = runs[key]
                own = min(p[0] for p in placed if p[2] == src)
                t = min(n // 2 + 3 * step, own, n - 1)              # units behind the boundary: their aliases start at 0
                for less in range(8):                               # (displaced: by another distance than the straddler of the boundary in front)
                    o = boundary + t - less * step - n
                    o -= (o - off) % step
                    if o < boundary < o + n and not _own_alias(o, o + n, src, placed, moduli, weak):
                        if best is None or o + n > best[0] + best[1]:
                            best = (o, n, src, key)
                        break
            if best is not None:
                if weak is not None:
                    displaced.append(best[3])
                break
        assert best is not None, "no run can straddle %d" % boundary
        o, n, src, key = best
        placed.append([o, o + n, src, key])
        out[key] = o
        at = o + n
        for key in sorted((k for k in keys if k != best[3]), key=lambda k: (-k[1], -k[0])):
            src, n, off = runs[key]
            o = at + gap
            o += (off - o) % step
            while True:
                bump = _own_alias(o, o + n, src, placed, moduli)
                if not bump:
                    break
                o += (bump + step - 1) // step * step
            placed.append([o, o + n, src, key])
            out[key] = o
            at = o + n
    check_aliases(placed, moduli, data, displaced)
    return out, displaced


def check_aliases(placed, moduli, data, displaced=()):
    """the alias rule, and that no two runs overlap: placed = [[lo, hi, source, key]]"""
    order = sorted(placed)
    for a, b in zip(order, order[1:]):
        assert a[1] <= b[0], (a, b)
    for lo, hi, src, key in placed:
        assert not _own_alias(lo, hi, src, placed, moduli, data if key in displaced else None), \
            "run %r at %d has an alias on its own source" % (key, lo)


def _slot_alias_ok(slot, slots):
    """every alias of the PCM slot [lo, hi, source, ...] modulo E30, E31 and E32 takes in a word that is no word of a slot of the same
    source in `slots`: poison, or another source's"""
    lo, hi, src = slot[:3]
    for m in (E30, E31, E32):
        for a, b, _ in _mod_pieces(lo, hi, m):
            if sum(min(b, q[1]) - max(a, q[0]) for q in slots if q[2] == src and a < q[1] and q[0] < b) >= b - a:
                return False
    return True


class FarContract:
    """contract(level) laid out sparsely, so that every offset a descriptor hands to a plan leaves 32 bits (include/acm_hip.h gives each
    of them 64): the same sources, copies, descriptors, shapes, residues modulo 64 (every run moves by a multiple of 64 words) and guards.

      * index arena (int16 elements): copy 0 of every source where contract(level) has it; one copy 1 straddles E31 = 2^31 elements (byte
        2^32) and the other copies 1 follow it; one copy 2 straddles E32 = 2^32 and the copies 3 and the other copies 2 follow that.  8
        words of IDX_POISON in front of and behind every copy, FILL bytes everywhere else;
      * header arena: the runs of copies 0 and 1 where contract(level) has them, one run of copies 2 / 3 straddles entry 2^29 (byte 2^32),
        the others follow, a poison header in front of each;
      * the alias rule (lay_far): for every moved copy and header run, the places its offsets come to with their high bits dropped - modulo
        E31 and E32, headers modulo 2^29 - hold the fill or ANOTHER source's data, unit by unit: a kernel that drops high bits on a read
        computes wrong samples.  That decides which copy straddles (the units behind a boundary alias to the arena's start, where copy 0 of
        source A begins at word 8: never A's) and how far behind E32 the copies 3 begin: not within 64 words of it, where their aliases
        would lie on copy 0 of their own source, but at the first place behind the straddling copy 2 whose aliases are clear of it.  With two
        sources B straddles both E31 and E32, and B's rows in front of E32 alias to B's rows in front of E31: there the rule is that
        the alias holds the same source's data DISPLACED - other rows, checked on the data (.idx_displaced names such copies);
      * descriptors: contract(level)'s, dealt into FAR_RUNS consecutive runs (descriptor j of a source into run (j + j / 4) mod 4: every
        run has descriptors from row 0 and windows, of every source and copy).  Run 0 is near; in runs 1, 2, 3 a slot of at least a tile
        straddles E30, E31, E32 - its last words lie behind the boundary - and the slot behind it begins within 64 elements behind the
        boundary.  The same element offsets serve int16 and float32 (E30 floats are byte 2^32), pcm_words = E32 + a tail;
      * PCM aliases (modulo E30, E31 and E32): run 0 begins behind the longest tail a run has behind its boundary, so the words behind a
        boundary alias to poison; the alias of a whole slot in front of a boundary always takes in a word that is poison or another
        source's (slots are 8 guard words apart): a kernel that drops high bits on a write dirties poison.

    Nothing of arena size exists on the host: .idx_pieces / .hdr_pieces are [(offset, array)], .idx_words / .hdr_entries / .pcm_words the
    sizes, and expected / describe_word work on slots."""

    def __init__(self, level):
        near = self.near = contract(level)
        self.level, self.cols, self.T, self.sources = level, near.cols, near.T, near.sources
        cols, nsrc = self.cols, len(self.sources)
        keys = [(k, c) for c in range(COPIES) for k in range(nsrc)]

        runs = {(k, c): (k, s.nrows * cols, s.idx_off[c]) for k, s in enumerate(self.sources) for c in range(COPIES)}
        self.idx_off, self.idx_displaced = lay_far(runs, [(E31, [q for q in keys if q[1] == 1]), (E32, [q for q in keys if q[1] >= 2])], 64, 16,
                                                   (E31, E32), {k: s.st.idx[:s.nrows * cols] for k, s in enumerate(self.sources)})
        guard = np.full(8, IDX_POISON, dtype=np.int16)
        self.idx_pieces = sorted((self.idx_off[(k, c)] - 8, np.concatenate([guard, self.sources[k].st.idx[:runs[(k, c)][1]], guard])) for k, c in keys)
        self.idx_words = max(o + a.size for o, a in self.idx_pieces) + 56

        hruns = {(k, c): (k, s.st.info.blocks, s.hdr_off[c]) for k, s in enumerate(self.sources) for c in range(COPIES)}
        self.hdr_off, self.hdr_displaced = lay_far(hruns, [(H29, [q for q in keys if q[1] >= 2])], 2, 1, (H29,),
                                                   {k: s.st.hdr[:s.st.info.blocks] for k, s in enumerate(self.sources)})
        front = np.array([HDR_POISON], dtype=np.uint32)
        self.hdr_pieces = sorted((self.hdr_off[(k, c)] - 1, np.concatenate([front, self.sources[k].st.hdr[:hruns[(k, c)][1]]]).astype(np.uint32))
                                 for k, c in keys)
        self.hdr_entries = max(o + len(a) for o, a in self.hdr_pieces) + 3
        self._idx_runs = [[self.idx_off[q], self.idx_off[q] + runs[q][1], q[0], q] for q in keys]
        self._hdr_runs = [[self.hdr_off[q], self.hdr_off[q] + hruns[q][1], q[0], q] for q in keys]

        # descriptors: dealt into runs, each run laid out by the near rule from a multiple of 64
        first = {}
        for i, k in enumerate(near.desc_source):
            first.setdefault(k, i)
        run_of = [((i - first[k]) + (i - first[k]) // 4) % FAR_RUNS for i, k in enumerate(near.desc_source)]
        # a run's slots by the near rule from a multiple of 64; runs 1 to 3 begin with whichever of their descriptors lets a slot straddle
        order, rel = [], []
        self.straddler, base = {}, {}
        tails, laid = [0], []
        for r, boundary in enumerate((0, E30, E31, E32)):
            members = [i for i in range(len(near.descs)) if run_of[i] == r]
            for rot in range(len(members) if r else 1):
                seq, at0 = members[rot:] + members[:rot], len(order)
                rl, end = [], 0
                for q, i in enumerate(seq):
                    rl.append(_next_at(end, 8, 8 * ((at0 + q) % 8)))
                    end = rl[-1] + near.descs[i].n_emit
                for q in range(len(seq) - 1 if r else 0):
                    ne = near.descs[seq[q]].n_emit
                    d = (rl[q] + ne) % 64                       # words of the slot behind the boundary
                    if ne >= self.T * cols and ne > d >= 1 and 64 >= (rl[q + 1] - rl[q] - ne) + d:
                        at = boundary + d - (rl[q] + ne)
                        trial = [[at + o, at + o + near.descs[i].n_emit, near.desc_source[i], i] for o, i in zip(rl, seq)]
                        if all(_slot_alias_ok(t, laid + trial) for t in trial):         # (the slots in front of E31 alias to those in front of E30)
                            self.straddler[r], base[r] = at0 + q, at
                            laid += trial
                            break
                if not r or r in self.straddler:
                    break
            assert not r or r in self.straddler, "level %d: no slot of run %d can straddle its boundary" % (level, r)
            if r:
                assert base[r] % 64 == 0
                tails.append(base[r] + end - boundary)
            order += seq
            rel += rl
        self.desc_source = [near.desc_source[i] for i in order]
        self.desc_copy = [near.desc_copy[i] for i in order]
        self.desc_run = [run_of[i] for i in order]
        self.near_index = order
        base[0] = (max(tails) + 64 + 63) // 64 * 64
        self.descs, plist = [], []
        for j, i in enumerate(order):
            d, k, c = near.descs[i], self.desc_source[j], self.desc_copy[j]
            self.descs.append(capi.StreamDesc(idx_off=self.idx_off[(k, c)], hdr_off=self.hdr_off[(k, c)], pcm_off=base[self.desc_run[j]] + rel[j],
                                              n_emit=d.n_emit, level=level, rows=d.rows, nrows=d.nrows, row_begin=d.row_begin))
            plist += [capi.Patch(p.sample, p.value, j) for p in self.sources[k].patches]
        self.patches = (capi.Patch * len(plist))(*plist) if plist else None
        self.pcm_words = self.descs[-1].pcm_off + self.descs[-1].n_emit + 64
        self.slots = [[d.pcm_off, d.pcm_off + d.n_emit, k, j] for j, (d, k) in enumerate(zip(self.descs, self.desc_source))]
        self._starts = np.array([d.pcm_off for d in self.descs], dtype=np.int64)
        self.check_pcm_aliases()

    def check_pcm_aliases(self):
        """slots ascend 8 words and more apart; what lies behind E30 / E31 / E32 in a far run aliases into the poison in front of run 0;
        the alias of every slot takes in a word that is poison or another source's slot"""
        for a, b in zip(self.slots, self.slots[1:]):
            assert a[1] + 8 <= b[0], (a, b)
        lead = self.slots[0][0]
        for lo, hi, src, j in self.slots:
            boundary = (0, E30, E31, E32)[self.desc_run[j]]
            assert hi - boundary <= lead - 8 or not boundary, "slot %d ends %d words behind its boundary, run 0 begins at %d" % (j, hi - boundary, lead)
            assert _slot_alias_ok([lo, hi, src, j], self.slots), "an alias of slot %d lies wholly on slots of its own source" % j

    def whole_copy_descs(self):
        """as Contract.whole_copy_descs, in the same order, with the far offsets"""
        whole, at = [], {}
        for k, s in enumerate(self.sources):
            for c in range(COPIES):
                at[(k, c)] = len(whole)
                whole.append(capi.StreamDesc(idx_off=self.idx_off[(k, c)], hdr_off=self.hdr_off[(k, c)], pcm_off=0, n_emit=s.nrows * self.cols,
                                             level=self.level, rows=s.rows, nrows=s.nrows, row_begin=0))
        return whole, [at[(k, c)] for k, c in zip(self.desc_source, self.desc_copy)]

    def expected(self, i, fmt):
        d = self.descs[i]
        lo = d.row_begin * self.cols
        return self.sources[self.desc_source[i]].pcm(fmt)[lo:lo + d.n_emit]

    def gaps(self):
        """[lo, hi) of everything in the PCM arena that is no slot, ascending"""
        edges = [0] + [e for lo, hi, _, _ in self.slots for e in (lo, hi)] + [self.pcm_words]
        return [(a, b) for a, b in zip(edges[::2], edges[1::2]) if b > a]

    def describe(self, i):
        d = self.descs[i]
        return "desc %d (level %d, source %s copy %d, run %d, idx_off %d hdr_off %d pcm_off %d, row_begin %d, n_emit %d)" % (
            i, d.level, self.sources[self.desc_source[i]].name, self.desc_copy[i], self.desc_run[i], d.idx_off, d.hdr_off, d.pcm_off,
            d.row_begin, d.n_emit)

    def aliases_of(self, w):
        """the slots and boundaries word w of the PCM arena is an alias of: text, or ''"""
        out = []
        for m, name in ((E30, "E30"), (E31, "E31"), (E32, "E32")):
            for k in range(1, (self.pcm_words - 1 - w) // m + 1):
                v = w + k * m
                j = int(np.searchsorted(self._starts, v, side="right")) - 1
                if j >= 0 and v < self.slots[j][1]:
                    out.append("the alias modulo %s of sample %d of desc %d" % (name, v - self.slots[j][0], j))
            if w < 64:
                out.append("%d words behind the alias of boundary %s" % (w, name))
        return "; ".join(out)

    def describe_word(self, w):
        """where word w of the PCM arena lies, the way Contract.check reports a dirty guard word: the descriptor in front of it and how far
        behind that descriptor's n_emit, the descriptor behind it - and every slot or boundary the word is an alias of"""
        i = int(np.searchsorted(self._starts, w, side="right")) - 1
        if i < 0:
            text = "word %d lies %d words in front of the first slot" % (w, self._starts[0] - w)
        elif w < self.slots[i][1]:
            text = "word %d is sample %d of %s" % (w, w - self.slots[i][0], self.describe(i))
        else:
            behind = ", %d words in front of desc %d" % (self._starts[i + 1] - w, i + 1) if i + 1 < len(self.slots) else ""
            text = "word %d lies %d words behind the n_emit of %s%s" % (w, w - self.slots[i][1], self.describe(i), behind)
        also = self.aliases_of(w)
        return text + ("; it is " + also if also else "")


@functools.lru_cache(maxsize=2)
def far_contract(level):
    """the level's far arenas, built once and shared (read-only) by the tests of that level"""
    return FarContract(level)


B32 = 1 << 32                                   # bytes
PAIR_FILL, BLOB_FILL, CHUNK_FILL = 0x01, FILL, 0x00


class FarForm:
    """The byte-plane or the packed form of every copy of every source of far_contract(level), relocated: built from contract(level)
    with capi.mform_streams / capi.pack_streams, then

      * .blob_pieces [(byte offset, bytes)]: the regions of copies 0 and 1 where the near arena has them, one region of copies 2 / 3
        astride byte 2^32, the others behind it (lay_far: the same alias rule, modulo 2^32 bytes);
      * .table_pieces [(entry offset, entries)]: the pair table / chunk table likewise about the entry that is byte 2^32 (pair entry
        2^30, chunk record 2^29), the blob offsets inside the entries rebased by what their region moved (the pair entry's 64-byte-unit
        field, the chunk record's blob_off16: both reach 64 GB);
      * .streams: the PackedStream beside every descriptor (none for a source with H1 patches).

    Outside the pieces the blob holds BLOB_FILL bytes.  The pair table holds PAIR_FILL bytes: an entry 0x01010101, which names a place
    269 MB into the blob - inside the allocation, behind everything near, fill; the chunk table holds zeros: unused records.  A kernel
    that drops high bits of a table index or of a blob offset decodes fill or another source and never reads outside the arenas."""

    def __init__(self, fc, form):
        L = capi.lib()
        near, level = fc.near, fc.level
        whole, _ = near.whole_copy_descs()
        arena = capi.mform_streams(near.idx, whole) if form == "byteplane" else capi.pack_streams(near.idx, whole)
        keys = [(k, c) for k in range(len(fc.sources)) for c in range(COPIES)]          # the order of whole_copy_descs
        have = [w for w, p in enumerate(arena.streams) if p.ntiles]
        assert have == list(range(len(keys))), "level %d: a copy without a %s form" % (level, form)
        self.form, self.unit = form, 4 if form == "byteplane" else 8
        self.table_boundary = B32 // self.unit
        if form == "byteplane":
            blob, table = arena.data[:arena.data.size - 64], arena.pairs
            count = [int(L.acmhip_mform_pairs(p.ntiles * L.acmhip_mform_tile_rows(level))) for p in arena.streams]
            start = [int(table[p.chunk_off] >> 2) * 64 for p in arena.streams]
            step = 64
        else:
            blob, table = arena.blob, arena.chunks
            count = [p.ntiles * L.acmhip_packed_slots(level) for p in arena.streams]
            start = []
            for p, n in zip(arena.streams, count):
                c = table[p.chunk_off:p.chunk_off + n]
                start.append(int(c["blob_off16"][c["kind"] != 0].min()) * 16)
            start[0], step = 0, 16
        end = start[1:] + [blob.size]
        assert all(a < b for a, b in zip(start, end)), "the regions of the near blob ascend"
        tab_at = [p.chunk_off for p in arena.streams]
        region = {q: blob[start[w]:end[w]] for w, q in enumerate(keys)}
        rel = {}
        for w, q in enumerate(keys):            # the entries with their blob offsets counted from the region's start: alike in every copy
            e = table[tab_at[w]:tab_at[w] + count[w]].copy()
            if form == "byteplane":
                e -= np.uint32((start[w] // 64) << 2)
            else:
                e["blob_off16"][e["kind"] != 0] -= start[w] // 16
            rel[q] = e
        for k in range(len(fc.sources)):
            assert all(np.array_equal(region[(k, 0)], region[(k, c)]) and np.array_equal(rel[(k, 0)], rel[(k, c)]) for c in range(COPIES))
        far = [q for q in keys if q[1] >= 2]
        plain = [k for k, s in enumerate(fc.sources) if not s.patches]          # (no plan reads the form of a source with H1 patches)
        self.blob_off, self.blob_displaced = lay_far({q: (q[0], region[q].size, start[w]) for w, q in enumerate(keys)}, [(B32, far)], step, 64, (B32,),
                                                     {k: region[(k, 0)] for k in range(len(fc.sources))}, plain)
        self.table_off, self.table_displaced = lay_far({q: (q[0], count[w], tab_at[w]) for w, q in enumerate(keys)}, [(self.table_boundary, far)], 1, 0,
                                                       (self.table_boundary,),
                                                       {k: rel[(k, 0)].view(np.uint32).reshape(count[4 * k], -1) for k in range(len(fc.sources))}, plain)
        self.blob_pieces = sorted((self.blob_off[q], region[q]) for q in keys)
        self.table_pieces = []
        for q in keys:
            e = rel[q].copy()
            if form == "byteplane":
                e += np.uint32((self.blob_off[q] // 64) << 2)
                assert int(e.max()) >> 2 == (self.blob_off[q] + int(rel[q].max() >> 2) * 64) // 64
            else:
                e["blob_off16"][e["kind"] != 0] += self.blob_off[q] // 16
            self.table_pieces.append((self.table_off[q], e))
        self.table_pieces.sort(key=lambda t: t[0])
        self.blob_bytes = max(o + a.size for o, a in self.blob_pieces) + 256
        self.table_entries = max(o + len(a) for o, a in self.table_pieces) + 32        # (the kernels fetch whole groups of pair entries)
        self.table_bytes = self.table_entries * self.unit
        if form == "byteplane":
            named = (0x01010101 * PAIR_FILL >> 2) * 64
            assert max(o + a.size for o, a in self.blob_pieces if o < B32 // 2) < named and named + (4 << level) + 64 < B32 // 2
        patched = [bool(fc.sources[k].patches) for k in fc.desc_source]
        self.streams = [capi.PackedStream(self.table_off[(k, c)], 0 if patched[j] else arena.streams[4 * k + c].ntiles, arena.streams[4 * k + c].form)
                        for j, (k, c) in enumerate(zip(fc.desc_source, fc.desc_copy))]
        self.ntiles = {q: arena.streams[w].ntiles for w, q in enumerate(keys)}
        self.count = {q: count[w] for w, q in enumerate(keys)}


@functools.lru_cache(maxsize=2)
def far_form(level, form):
    return FarForm(far_contract(level), form)
