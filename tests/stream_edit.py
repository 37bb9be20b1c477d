"""Editing the bits of a synthetic stream, without a device: single-bit flips, and symbols and codes written where one wants them in a
stream that uses one ternary filler alone.  Shared by tests/test_gpu_batch_index.py (which re-exports these names for
tests/decode_index.py and tests/test_decode_index.py) and tests/damaged_streams.py.

Every expectation here is the host's acm_index_file, computed once per file image."""
import ctypes as C

import numpy as np

from helpers import make_stream
from libacm_amd import capi, synth

ACM_ERR_CORRUPT = -6
TERNARY = (19, 22, 29)

_host = {}


def host_index(data):
    """acm_index_file for these bytes, computed once -> (rc, blocks, end_status, marks[0 .. blocks], promised, in_S)"""
    data = bytes(data)
    if data not in _host:
        a = capi._as_u8(data)
        rc, info = capi.probe(a)
        room = promised = 0
        if rc == 0:
            bl = info.rows * info.cols
            promised = (info.total_values + bl - 1) // bl
            room = min(promised, (max(0, a.size - info.header_bytes) * 8 + 8) // (20 + 5 * info.cols) + 1)
        marks = np.zeros(room + 1, dtype=capi.BLOCK_MARK_DT)
        st = capi.StageInfo()
        rc = capi.lib().acm_index_file(a.ctypes.data, a.size, 0, marks.ctypes.data, room, C.byref(st))
        supported = capi.lib().acmk_parse_supported
        supported.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]
        in_s = bool(rc == 0 and st.end_status == 0 and st.blocks == promised and promised >= 1 and int(marks[st.blocks]["bit"]) <= 8 * a.size and
                    supported(st.level, st.rows, a.size, promised))
        _host[data] = (rc, st.blocks, st.end_status, marks[:st.blocks + 1] if rc == 0 else marks[:0], promised, in_s)
    return _host[data]


def single(code, level, rows, nblocks=3, seed=0, **kw):
    return make_stream(1000 * code + 10 * level + seed, level, rows, nblocks, mix=synth.MIX_SINGLE, single_code=code, **kw)


def flip(data, bit):
    b = bytearray(data)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def read_bits(data, bit, n):
    return (int.from_bytes(data[bit >> 3:(bit + n + 7 >> 3) + 1], "little") >> (bit & 7)) & ((1 << n) - 1)


def write_bits(data, bit, n, value):
    """`data` with the n bits from `bit` on set to `value` (LSB first)"""
    f = data
    for k in range(n):
        if (read_bits(f, bit + k, 1) ^ (value >> k)) & 1:
            f = flip(f, bit + k)
    assert read_bits(f, bit, n) == value and len(f) == len(data)
    return f


def find_flips(data, block, want_corrupt=1, want_alive=1, limit=400):
    """single-bit flips inside block `block` of a clean stream, searched on the CPU: the first `want_corrupt` the host index ends with
    ACM_ERR_CORRUPT on and the first `want_alive` it survives (same blocks, clean end)"""
    rc, blocks, end, marks, promised, s = host_index(data)
    assert s and block < blocks
    lo, hi = int(marks[block]["bit"]) + 20, int(marks[block + 1]["bit"])
    corrupt, alive = [], []
    for bit in range(lo, min(hi, lo + limit)):
        f = flip(data, bit)
        r = host_index(f)
        if r[2] == ACM_ERR_CORRUPT and len(corrupt) < want_corrupt:
            corrupt.append(f)
        elif r[5] and len(alive) < want_alive:
            alive.append(f)
        if len(corrupt) == want_corrupt and len(alive) == want_alive:
            break
    assert len(corrupt) == want_corrupt, (block, len(corrupt))
    return corrupt, alive


# ---- symbols out of range inside a ternary column -------------------------------------------------------------------------------
# In a stream that uses one ternary filler alone every column has the same length, whatever its symbols are: 5 bits of code and
# `groups` groups of `width` bits.  So a change of the payload bits moves no column and no block, every code stays what it was, and
# the one reason left for the host reader to end the stream in that block is the symbol itself (decode.c:413, :439, :465).  A walk that
# only skips such a column by its length runs through to the last block and hands back a clean index: both the marks and the counts
# of test_gpu_batch_index.run() then differ from the host's.

TERN_WIDTH = {19: 5, 22: 7, 29: 7}
TERN_LIMIT = {19: 27, 22: 125, 29: 121}


def tern_groups(code, rows):
    return (rows + 1) // 2 if code == 29 else (rows + 2) // 3


def group_bit(base, code, level, rows, block, col, g):
    """where group `g` of column `col` of block `block` starts in a single-code ternary stream"""
    marks = host_index(base)[3]
    width, groups = TERN_WIDTH[code], tern_groups(code, rows)
    column = 5 + groups * width
    assert int(marks[block + 1]["bit"]) - int(marks[block]["bit"]) == 20 + (column << level)       # (the geometry is what this test thinks)
    assert 0 <= col < 1 << level and 0 <= g < groups
    at = int(marks[block]["bit"]) + 20 + col * column
    assert read_bits(base, at, 5) == code
    return at + 5 + g * width


def with_symbol(base, code, level, rows, block, col, g, value):
    """`base` with that group set to `value`, checked against the host reader: a value in range leaves the index as it was (the stream stays
    in S), one out of range ends the stream in that very block with ACM_ERR_CORRUPT, every earlier mark unchanged"""
    width = TERN_WIDTH[code]
    bit = group_bit(base, code, level, rows, block, col, g)
    f = base
    for k in range(width):
        if (read_bits(f, bit + k, 1) ^ (value >> k)) & 1:
            f = flip(f, bit + k)
    assert read_bits(f, bit, width) == value and len(f) == len(base)
    check_symbol_change(base, f, block, value >= TERN_LIMIT[code])
    return f


def check_symbol_change(base, f, block, bad):
    rc, blocks, end, marks, promised, s = host_index(f)
    want = host_index(base)
    if bad:
        assert (rc, blocks, end, s) == (0, block, ACM_ERR_CORRUPT, False), (rc, blocks, end, block)
        assert np.array_equal(marks[:block], want[3][:block]) and int(marks[block]["bit"]) == int(want[3][block]["bit"])
    else:
        assert s and (rc, blocks, end) == want[:3] and np.array_equal(marks, want[3])


def symbol_flips(base, code, level, rows, block, cols, groups):
    """single-bit flips inside the symbol bits of block `block`, searched over the given columns and groups: the first that puts its group
    out of range and the first that leaves it in range -> (bad stream, surviving stream)"""
    width, lim = TERN_WIDTH[code], TERN_LIMIT[code]
    found = {}
    for col in cols:
        for g in groups:
            bit = group_bit(base, code, level, rows, block, col, g)
            v = read_bits(base, bit, width)
            for k in range(width):
                bad = (v ^ (1 << k)) >= lim
                if bad not in found:
                    found[bad] = flip(base, bit + k)
                    check_symbol_change(base, found[bad], block, bad)
            if len(found) == 2:
                return found[True], found[False]
    raise AssertionError(("no such flip", code, rows, block))
