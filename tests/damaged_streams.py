"""A population of DAMAGED streams of real size, and what the compiled reference does with each of them.  Shared by
tests/test_damaged_streams.py and tests/test_gpu_damaged_streams.py.  Deterministic (seeded), no device.

A damaged stream has three observable sides (libacm.h promises the reference's behaviour on all of them): the bytes delivered before
an error, the call that returns it, and what a caller that keeps calling gets afterwards - the reference parses on from wherever its
bit reader stood when decode_block failed (decode.c:580-611, :826-846; acm_read_loop swallows an error behind some output,
util.c:258-277).  The hand-assembled F3_corrupt goldens are a few dozen bytes with nothing decodable behind the error; here every
base stream has blocks behind the damage.

Base streams: prime_table=1 (block 0 writes the whole amplitude table: a damaged header or code may then make the reference read
stale entries, never uninitialised memory), ragged total_values, mono and stereo, one WAVC file, both mixes - the smallest shapes
that reach every parser path - and streams of one filler alone for the three ternary codes and two k codes.

Damage: one or three bit flips and truncations at random places (flips behind the first third of the file, as
test_oracle_vs_ref.py::test_bit_flips has it), an out-of-range ternary symbol written on purpose (first, middle, last whole and
partial group of a column; first, a middle and the last block), an invalid filler code written into a chosen column.

answers() is the reference's side, through helpers.RefAnswers (digests, never PCM): replayed from tests/golden/ref_answers.json,
recorded by tests/golden/make_golden_ref_answers.py."""
from collections import namedtuple

import numpy as np

import oracle_api as O
from helpers import RefAnswers, make_stream, sha
from libacm_amd import synth
from stream_edit import TERN_LIMIT, TERN_WIDTH, TERNARY, flip, group_bit, host_index, read_bits, single, tern_groups, with_symbol, write_bits

KEY = "test_damaged_streams::population"
LOOP_STEPS = (8192, 3 * 4096 + 2, 1 << 20)      # acm_read_loop request sizes; the first is the one every case's main record uses
TINY_STEP, TINY_SAMPLES = 2, 1000               # 2-byte reads: on the shapes of at most 1000 samples only (some 20 ms per case)

# (level, rows, blocks, channels, mix, wavc)
SHAPES = [(0, 7, 40, 1, 0, 0), (2, 64, 30, 2, 1, 0), (3, 5, 12, 1, 0, 0), (5, 33, 6, 2, 0, 0), (6, 8, 200, 1, 1, 0), (7, 16, 6, 2, 0, 0),
          (8, 255, 2, 1, 0, 0), (9, 3, 5, 1, 1, 1), (9, 16, 8, 2, 0, 0), (11, 2, 4, 1, 1, 0), (13, 1, 4, 1, 0, 0)]
SINGLE_LEVEL, SINGLE_ROWS, SINGLE_BLOCKS = 2, 17, 10            # 17 rows: the last group of a ternary column is a partial one
SINGLE_K = (17, 24)

Base = namedtuple("Base", "name data level rows blocks channels single")
# kind: clean / flip1 / flip3 / cut / symbol / code; code: the ternary filler of a `symbol` case; at: the first damaged bit of the file (a cut:
# the first missing one; None: clean)
Case = namedtuple("Case", "name base kind data code at")

_population = None
_answers = None


def bases():
    out = []
    for k, (lv, rows, nb, ch, mix, wavc) in enumerate(SHAPES):
        data = make_stream(7000 + k, lv, rows, nb, channels=ch, cut=3, mix=mix, wavc=wavc, prime_table=1)
        out.append(Base("L%d_r%d%s%s" % (lv, rows, "_stereo" if ch == 2 else "", "_wavc" if wavc else ""), data, lv, rows, nb, ch, 0))
    for code in TERNARY + SINGLE_K:
        data = single(code, SINGLE_LEVEL, SINGLE_ROWS, nblocks=SINGLE_BLOCKS, seed=3, cut=3, prime_table=1)
        out.append(Base("single%d" % code, data, SINGLE_LEVEL, SINGLE_ROWS, SINGLE_BLOCKS, 1, code))
    return out


def samples(base):
    return base.blocks * (base.rows << base.level)


def block_bit(base, block):
    return int(host_index(base.data)[3][block]["bit"])


def damaged_block(case):
    """the block of the clean stream that holds the first damaged bit (None: clean; -1: the file header)"""
    if case.at is None:
        return None
    bits = host_index(case.base.data)[3]["bit"].astype(np.int64)
    return int(np.searchsorted(bits, case.at, side="right")) - 1


def random_cases(base, rng, nflip1, nflip3, ncut, head_cut):
    n = len(base.data)
    out = []
    for kind, count, nbits in (("flip1", nflip1, 1), ("flip3", nflip3, 3)):
        for k in range(count):
            f, bits = base.data, []
            for _ in range(nbits):
                bits.append(8 * int(rng.integers(n // 3, n)) + int(rng.integers(0, 8)))
                f = flip(f, bits[-1])
            if f != base.data:                  # (three flips may undo each other)
                out.append(Case("%s:%s:%d" % (base.name, kind, k), base, kind, f, 0, min(bits)))
    for k, cut in enumerate([int(rng.integers(0, n)) for _ in range(ncut)] + ([7] if head_cut else [])):
        out.append(Case("%s:cut:%d" % (base.name, k), base, "cut", base.data[:cut], 0, 8 * cut))
    return out


def symbol_cases(base):
    """an out-of-range symbol - the limit itself and all ones in turn - in the first, a middle, the last whole and the partial group of a
    column, in the first two, a middle and the last two blocks, every column in turn"""
    code, lv, rows = base.single, base.level, base.rows
    groups, lim, top = tern_groups(code, rows), TERN_LIMIT[code], (1 << TERN_WIDTH[code]) - 1
    assert rows % (2 if code == 29 else 3)                  # (the last group is partial)
    out, k = [], 0
    for block in (0, 1, base.blocks // 2, base.blocks - 2, base.blocks - 1):
        for g in (0, groups // 2, groups - 2, groups - 1):
            col = k % (1 << lv)
            value = (lim, top, lim + 1)[k % 3]
            f = with_symbol(base.data, code, lv, rows, block, col, g, value)
            at = group_bit(base.data, code, lv, rows, block, col, g)
            out.append(Case("%s:symbol:b%d:c%d:g%d:%d" % (base.name, block, col, g, value), base, "symbol", f, code, at))
            k += 1
    return out


def code_cases(base, k0):
    """one of the six invalid codes in place of a column's code: column 0 of a first, a middle and the last block (a block's first code
    is 20 bits behind its mark) and, where the columns have one length, an inner and the last column too"""
    out = []
    where = [(b, 0) for b in (0, base.blocks // 2, base.blocks - 1)]
    if base.single in TERNARY:
        where += [(1, 1), (base.blocks // 2, (1 << base.level) - 1), (base.blocks - 2, 2)]
    for k, (block, col) in enumerate(where):
        bad = synth.BAD_CODES[(k0 + k) % 6]
        at = block_bit(base, block) + 20 if col == 0 else group_bit(base.data, base.single, base.level, base.rows, block, col, 0) - 5
        if base.single:
            assert read_bits(base.data, at, 5) == base.single
        f = write_bits(base.data, at, 5, bad)
        assert host_index(f)[1:3] == (block, -6), (base.name, block, col)
        out.append(Case("%s:code:b%d:c%d:%d" % (base.name, block, col, bad), base, "code", f, 0, at))
    return out


def population():
    global _population
    if _population is None:
        cases = []
        for k, base in enumerate(bases()):
            rng = np.random.default_rng([0xDA3A, k])
            cases.append(Case("%s:clean" % base.name, base, "clean", base.data, 0, None))
            cases += random_cases(base, rng, 12, 6, 4, head_cut=k % 4 == 0)       # (a few files that end inside their header)
            cases += code_cases(base, k)
            if base.single in TERNARY:
                cases += symbol_cases(base)
        _population = cases
    return _population


# ---- one stream through any libacm.h-shaped wrapper (O.LibacmStream over the reference or the library, O.Oracle) --------------------

def loop_record(open_stream, data, step):
    """the looping decode: acm_read_loop with `step`-byte requests until one returns <= 0 -> [sha256, final status, words, raw_tell]"""
    s = open_stream(data)
    assert s.err == 0
    out = []
    while True:
        rc, b = s.read(step, loop=True)
        if rc <= 0:
            break
        out.append(b)
    pcm = b"".join(out)
    rec = [sha(pcm), rc, len(pcm) // 2, s.getter("raw_tell")]
    s.close()
    return rec


def plain_reads(open_stream, data, block_bytes, **fmt):
    """plain acm_read, a block at a time, until one returns <= 0 -> (reads that delivered, that call's status, the bytes).  This is the
    rule of the batch calls and the stagers (include/acm_hip.h, acm_stage_file): every block in front of the first error, nothing behind it.
    fmt: be / sgned of the reads"""
    s = open_stream(data)
    assert s.err == 0
    out = []
    while True:
        rc, b = s.read(block_bytes, **fmt)
        if rc <= 0:
            break
        out.append(b)
    s.close()
    return len(out), rc, b"".join(out)


def steps_of(case):
    return LOOP_STEPS + ((TINY_STEP,) if samples(case.base) <= TINY_SAMPLES else ())


def record(open_stream, case):
    """everything the tests compare, as recorded: [open status] for a file that does not open, else
    [0, [blocks before the first failing acm_read, that call's status, sha256 of those blocks], the looping decode at LOOP_STEPS[0],
     one entry per further request size: 0 where it equals the first, else its own record]"""
    s = open_stream(case.data)
    if s.err < 0:
        return [s.err]
    s.close()
    blocks, status, pcm = plain_reads(open_stream, case.data, 2 * (case.base.rows << case.base.level))
    loops = [loop_record(open_stream, case.data, step) for step in steps_of(case)]
    return [0, [blocks, status, sha(pcm)], loops[0]] + [0 if r == loops[0] else r for r in loops[1:]]


def expand(rec):
    """record() with the per-size records spelled out -> (first, [loop record per size of steps_of])"""
    return rec[1], [rec[2]] + [rec[2] if r == 0 else r for r in rec[3:]]


def ref_stream(data):
    return O.LibacmStream(O.ref_lib(), data)


def answers():
    """the compiled reference's record() of every case of population(), in order"""
    global _answers
    if _answers is None:
        ans = RefAnswers(KEY)
        _answers = [ans.ask(lambda c=c: record(ref_stream, c)) for c in population()]
        ans.done()
    return _answers


def first_error(rec):
    """(blocks delivered before it, status) of the first failing plain acm_read; status 0: the stream ended without one"""
    return rec[1][0], rec[1][1]
