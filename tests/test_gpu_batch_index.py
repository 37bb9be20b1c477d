"""acm_batch_index_files on the GPU (libacm_amd/csrc/acm_batch_index.cpp, acm_parse.hip: acm_index_scan_wave).

Every case is one call with ACM_BATCH_PARSE_DEVICE, compared item by item with the host's acm_index_file - never with the device
path itself.  The fallback to the host pool must not hide a broken kernel, so every case also counts: with S the streams the device
has to take - the host index ends clean (end_status 0), has the blocks the header promises, its last mark lies inside the file, and
acmk_parse_supported holds - the call must report device_indexed == |S| and host_indexed == n - |S|.  Every input is one the host
reader handles too; streams are a few KB, except where a case is about their length."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_stream
from libacm_amd import capi, synth
# the stream editors live in a device-free module; they stay importable from here (tests/decode_index.py, tests/test_decode_index.py)
from stream_edit import (ACM_ERR_CORRUPT, TERN_LIMIT, TERN_WIDTH, TERNARY, check_symbol_change, find_flips, flip, group_bit,  # noqa: F401
                         host_index, read_bits, single, symbol_flips, tern_groups, with_symbol)

pytestmark = pytest.mark.gpu


def run(dev, files, expect_all_device=None, **kw):
    """one call; every item equals the host index, and the device took exactly the streams it must take"""
    got, tm, status = capi.batch_index_files(dev, files, parse=capi.PARSE_DEVICE, return_status=True, **kw)
    assert len(got) == len(files)
    in_s = 0
    for i, f in enumerate(files):
        rc, blocks, end, marks, promised, s = host_index(f)
        in_s += s
        assert status[i] == rc, (i, status[i], rc)
        if rc != 0:
            assert len(got[i]) == 0, i
            continue
        assert (len(got[i]) - 1, got[i].end_status) == (blocks, end), (i, len(got[i]) - 1, got[i].end_status, blocks, end, s)
        assert np.array_equal(np.asarray(got[i]), marks), (i, s)
    print("n %d  |S| %d  device_indexed %d  host_indexed %d  groups %d  blocks %d  device_bytes %d"
          % (len(files), in_s, tm.device_indexed, tm.host_indexed, tm.groups, tm.blocks, tm.device_bytes))
    assert (tm.device_indexed, tm.host_indexed) == (in_s, len(files) - in_s)
    assert tm.blocks == sum(host_index(f)[1] for f in files)
    if expect_all_device is not None:
        assert (in_s == len(files)) == expect_all_device
    return got, tm


@pytest.mark.parametrize("level", [0, 2, 6, 7])
def test_every_filler_code(dev, level):
    """each of the 26 valid codes alone in a stream; rows on both sides of the walk_k_column<4> / <5> switch (16) and with partial ternary
    groups (1, 2, 16, 17, 100); one column, four, exactly one 64-column pass, two passes"""
    files = [single(code, level, rows) for code in synth.VALID_CODES for rows in (1, 2, 3, 16, 17, 100)]
    run(dev, files, expect_all_device=True)


def test_long_ternary_columns(dev):
    """a column longer than the walk's 65-dword window: 4095 rows of code 22 are 9555 bits"""
    files = [single(code, 2, 4095, nblocks=2) for code in TERNARY]
    run(dev, files, expect_all_device=True)


def test_window_reloads_and_block_counts(dev):
    """level 9, the speech mix: the 65-dword window is reloaded hundreds of times per block at 255 rows; 1 to 300 blocks per stream"""
    files = [make_stream(300 + nb + rows, 9, rows, nb, cut=(nb % 3) * 1234) for rows in (8, 255) for nb in (1, 2, 65, 300)]
    run(dev, files, expect_all_device=True)


def test_wavc_prefix(dev):
    files = [make_stream(400 + i, lv, 8, 4, wavc=1) for i, lv in enumerate((0, 5, 9))] + [make_stream(410, 7, 8, 4)]
    assert capi.probe(files[0])[1].header_bytes == 42
    got, tm = run(dev, files, expect_all_device=True)
    assert int(got[0][0]["bit"]) == 8 * 42


def test_h1_streams_stay_on_the_device(dev):
    """an index does not care about indices outside a block's amplitude range"""
    files = [make_stream(420 + i, lv, 16, 6, allow_out_of_range=1, pwr_min=0, pwr_max=3) for i, lv in enumerate((3, 7, 9))]
    assert any(capi.stage_file(f).info.npatches for f in files)
    run(dev, files, expect_all_device=True)


@pytest.mark.parametrize("rows", [16, 100])
def test_bad_ternary_symbols(dev, rows):
    """one bit flipped inside a symbol of a column the walk skips by its length, in the first, a middle and the last block: the first such
    flip from the block's first column on, from its fourth on and from its last column backwards.  Beside each a flip that leaves its group
    in range: that stream stays on the device.  (Few values of a 7-bit group are one bit away from 125 or 121, so the search may pass over
    some groups; test_ternary_limits writes the symbol it wants, the last and partial group of a column included.)"""
    level, nblocks = 3, 7
    files, nbad = [], 0
    for code in TERNARY:
        base = single(code, level, rows, nblocks=nblocks, seed=5)
        groups = tern_groups(code, rows)
        files.append(base)
        for block, cols in ((0, range(8)), (3, range(3, 8)), (6, range(7, -1, -1))):
            files += symbol_flips(base, code, level, rows, block, cols, range(groups))
            nbad += 1
    got, tm = run(dev, files)
    assert nbad == 9 and tm.host_indexed == nbad and tm.device_indexed == len(files) - nbad


@pytest.mark.parametrize("code", TERNARY)
def test_ternary_limits(dev, code):
    """the limit itself: 27 for code 19, 125 for code 22, 121 for code 29.  A group set to the limit and to all ones ends the stream, one set
    to the limit minus one does not; in the first group, a middle one and the last, partial one (17 rows: 6 groups of code 19 and 22, 9 of code 29)"""
    level, rows, nblocks = 3, 17, 4
    base = single(code, level, rows, nblocks=nblocks, seed=6)
    lim, top, last = TERN_LIMIT[code], (1 << TERN_WIDTH[code]) - 1, tern_groups(code, rows) - 1
    files, nbad = [base], 0
    for block, col, g in ((0, 0, 0), (1, 3, last), (2, 5, last // 2), (3, 7, last)):
        for value in (lim, top, lim - 1, 0):
            files.append(with_symbol(base, code, level, rows, block, col, g, value))
            nbad += value >= lim
    got, tm = run(dev, files)
    assert nbad == 8 and tm.host_indexed == nbad and tm.device_indexed == len(files) - nbad


def test_bad_symbol_in_a_late_column(dev):
    """level 7: 128 columns, two passes of 64.  The bad symbol sits in the last column of the first pass, the first of the second, one in the
    middle of the second and the very last, there in the last group"""
    level, rows, nblocks = 7, 17, 3
    files, nbad = [], 0
    for code in TERNARY:
        base = single(code, level, rows, nblocks=nblocks, seed=8)
        last = tern_groups(code, rows) - 1
        files.append(base)
        for block, col, g in ((0, 63, 1), (1, 64, 0), (1, 100, last // 2), (2, 127, last)):
            files.append(with_symbol(base, code, level, rows, block, col, g, TERN_LIMIT[code]))
            files.append(with_symbol(base, code, level, rows, block, col, g, TERN_LIMIT[code] - 1))
            nbad += 1
    got, tm = run(dev, files)
    assert nbad == 12 and tm.host_indexed == nbad and tm.device_indexed == len(files) - nbad


def test_bad_symbol_behind_the_window(dev):
    """4095 rows: a column of 6825 to 14336 bits against a window of 65 dwords (2080 bits).  The bad symbol sits in the second round of
    64 groups (still inside the window), in groups far behind the window that a lane has to fetch for itself, in the first lane's group of
    the last round and in the last group of the column (partial for code 29: 4095 is odd)"""
    level, rows, nblocks = 2, 4095, 2
    files, nbad = [], 0
    for code in TERNARY:
        base = single(code, level, rows, nblocks=nblocks)
        groups = tern_groups(code, rows)
        assert (groups - 1) * TERN_WIDTH[code] > 3 * 2080
        files.append(base)
        for block, col, g in ((0, 0, 70), (0, 1, 500), (0, 3, (groups - 1) // 64 * 64), (1, 2, groups // 2 + 13), (1, 3, groups - 1)):
            assert g < 128 or g * TERN_WIDTH[code] > 2080 + 32
            files.append(with_symbol(base, code, level, rows, block, col, g, TERN_LIMIT[code]))
            files.append(with_symbol(base, code, level, rows, block, col, g, TERN_LIMIT[code] - 1))
            nbad += 1
    got, tm = run(dev, files)
    assert nbad == 15 and tm.host_indexed == nbad and tm.device_indexed == len(files) - nbad


def test_bad_filler_codes(dev):
    """codes 0, 3, 24 and 29 are one bit away from the invalid 1 / 2 / 25 / 28 / 30 / 31 (decode.c:190-194)"""
    files = []
    for code in (0, 3, 24, 29):
        base = single(code, 4, 5, nblocks=5, seed=7)
        for block in (0, 2, 4):
            corrupt, alive = find_flips(base, block, want_alive=1)
            files += corrupt + alive
    got, tm = run(dev, files)
    assert tm.host_indexed >= 12


def test_truncation_at_every_byte(dev):
    whole = make_stream(500, 5, 4, 3)
    assert len(whole) < 600
    files = [whole[:n] for n in range(len(whole) + 1)]
    got, tm = run(dev, files)
    assert tm.device_indexed >= 1 and tm.host_indexed >= len(whole) - 1


def test_short_files(dev):
    """a header whose total_values promises more blocks than the file holds"""
    files = []
    for i, (lv, rows, nb, extra) in enumerate([(0, 5, 4, 1), (5, 8, 3, 2), (9, 4, 2, 40), (7, 16, 1, 100000)]):
        bl = rows << lv
        files.append(synth.generate(seed=synth.BASE_SEED + 520 + i, level=lv, rows=rows, nblocks=nb, total_values=(nb + extra) * bl))
    files.append(make_stream(530, 5, 8, 3))
    got, tm = run(dev, files)
    assert tm.host_indexed == 4 and tm.device_indexed == 1


@pytest.fixture(scope="module")
def ragged():
    """300 streams (more than 256: workgroups of four wavefronts, the last one partial), levels 0-13, ragged lengths, a few that are not clean"""
    files = []
    for i in range(300):
        lv = i % 14
        rows = [1, 3, 8, 16, 33][i % 5] if lv < 11 else [1, 2, 4][i % 3]
        files.append(make_stream(600 + i, lv, rows, 1 + (i * 7) % 6, cut=(i % 4) * 3, wavc=1 if i % 37 == 5 else 0))
    files[17] = b"not an acm file"
    files[101] = files[101][:len(files[101]) // 2]
    files[202] = b""
    return files


def test_ragged_batch_in_one_group_and_in_several(dev, ragged):
    one, tm1 = run(dev, ragged)
    assert tm1.groups == 1 and tm1.host_indexed == 3
    budget = tm1.h2d_bytes // 4
    many, tm4 = run(dev, ragged, max_group_bytes=budget)
    assert tm4.groups >= 3 and tm4.device_bytes < tm1.device_bytes
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) and a.end_status == b.end_status for a, b in zip(one, many))
    # one-file groups
    few, tm = run(dev, ragged[:9], max_group_bytes=1)
    assert tm.groups == 9


def test_second_call_on_the_same_handle(dev, ragged):
    """arenas are reused: a smaller batch after a larger one, other files in the same slots"""
    with capi.Device(0) as d2:
        run(d2, ragged)
        run(d2, ragged[200:240][::-1])
        run(d2, [ragged[3]])
        run(d2, [b"junk", b""])


def test_crop_through_a_device_built_index():
    import torch
    from libacm_amd import batch
    files = [make_stream(700 + i, lv, rows, 5) for i, (lv, rows) in enumerate(((5, 16), (8, 16), (9, 3), (11, 4)))] + [b"no acm"]
    dec = batch.GpuDecoder(0, parse=capi.PARSE_DEVICE, dtype=torch.int16)
    try:
        host = batch.build_index(files, threads=2)
        built = dec.build_index(files)
        assert dec.index_timing.device_indexed == 4 and dec.index_timing.host_indexed == 1
        via_kw = batch.build_index(files, decoder=dec)
        for a, b, c in zip(host, built, via_kw):
            assert np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(a), np.asarray(c))
            assert getattr(a, "end_status", None) == b.end_status == c.end_status       # (None: the file that is not ACM)
        windows = [(0, 0, 100), (1, 1000, 5000), (2, 77, 3000), (3, 4099, 9000), (4, 0, 10), (0, 33, 64)]
        want = dec.crop(files, windows, host)
        want = (want[0].cpu().numpy().copy(),) + tuple(want[1:])
        for index in (built, None):
            pcm, o, n, st = dec.crop(files, windows, index=index)
            pcm = pcm.cpu().numpy()
            assert (o, n, st) == want[1:]
            for k in range(len(windows)):
                assert np.array_equal(pcm[o[k]:o[k] + n[k]], want[0][o[k]:o[k] + n[k]]), k
    finally:
        dec.dev.close()
