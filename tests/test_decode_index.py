"""The block index as a by-product of the host stagers, without a device (libacm_amd/csrc/acm_stage.h: MarkSink, acmk_stage_marks;
acm_batch.cpp: acm_batch_prestage / acm_batch_prestaged_index).

Every file goes through every host stager the pool of acm_batch_decode can pick at its level - acm_stage_file (int16 rows),
acm_stage_file_mform (byte planes, levels 7-14), acm_stage_file + acmhip_pack_tiles (packed, levels 6-9) - and through
acm_batch_prestage; what comes back must be byte for byte what acm_index_file writes into a poisoned buffer of the same size: return
code, blocks, end_status, marks[0 .. blocks], and the poison behind them."""
import numpy as np
import pytest

from decode_index import BYTEPLANE, INT16, PACKED, check_hook, check_prestage, index_info, stage_marks, POISON
from helpers import make_stream
from libacm_amd import capi, synth
from test_gpu_batch_index import ACM_ERR_CORRUPT, TERN_LIMIT, TERNARY, find_flips, host_index, single, tern_groups, with_symbol

pytestmark = []         # (test_gpu_batch_index is imported for its helpers only: nothing here needs a device)


def check(files, levels_with=(INT16,)):
    check_hook(files, levels_with)
    check_prestage(files)


@pytest.mark.parametrize("rows", [1, 2, 3, 16, 17])
def test_every_filler_code(rows):
    """each valid code alone in a stream: level 2 (int16 only) and level 7, where all three stagers exist"""
    files = [single(code, level, rows) for code in synth.VALID_CODES for level in (2, 7)]
    check(files, (INT16, BYTEPLANE, PACKED))


@pytest.mark.parametrize("level", [0, 5, 7, 9, 13])
def test_levels(level):
    """a few blocks, and from level 7 on enough rows for whole tiles: the byte-plane stager writes its form while it parses there
    (mf_rows > 0) instead of falling back to acm_stage_file"""
    files = [make_stream(800 + level, level, 3, 4, cut=5), make_stream(810 + level, level, 16 if level < 13 else 2, 12 if level < 13 else 4),
             make_stream(820 + level, level, 1, 1), make_stream(830 + level, level, 8, 5, channels=2, cut=3)]
    if 7 <= level <= 12:
        assert capi.stage_file_mform(files[1])[5] > 0
    check(files, {0: (INT16,), 5: (INT16,), 7: (INT16, BYTEPLANE, PACKED), 9: (INT16, BYTEPLANE, PACKED), 13: (INT16, BYTEPLANE)}[level])


def test_wavc_prefix():
    files = [make_stream(840 + i, lv, 8, 4, wavc=1) for i, lv in enumerate((0, 5, 7, 9))]
    assert capi.probe(files[0])[1].header_bytes == 42 and int(host_index(files[2])[3][0]["bit"]) == 8 * 42
    check(files, (INT16, BYTEPLANE, PACKED))


def test_h1_stream():
    """indices outside the block's amplitude range: the stagers keep the patches of their one pass, the byte-plane one gives its
    attempt up and stages the plain way - the marks are the same"""
    files = [make_stream(850 + i, lv, 16, 6, allow_out_of_range=1, pwr_min=0, pwr_max=3) for i, lv in enumerate((3, 7, 9))]
    for f in files:
        assert index_info(f).npatches > 0 and capi.stage_file(f).info.npatches == index_info(f).npatches
    check(files, (INT16, BYTEPLANE, PACKED))


def test_bad_ternary_symbol():
    """a symbol out of range in the first, a middle and the last block: the stream ends there, the failed block's mark names its start"""
    level, rows, nblocks = 7, 17, 3
    files = []
    for code in TERNARY:
        base = single(code, level, rows, nblocks=nblocks, seed=8)
        last = tern_groups(code, rows) - 1
        for block, col, g in ((0, 63, 1), (1, 64, 0), (2, 127, last)):
            f = with_symbol(base, code, level, rows, block, col, g, TERN_LIMIT[code])
            assert host_index(f)[1:3] == (block, ACM_ERR_CORRUPT)
            files.append(f)
    check(files, (INT16, BYTEPLANE, PACKED))


def test_invalid_code():
    files = []
    for code in (0, 3, 24, 29):
        base = single(code, 7, 5, nblocks=5, seed=7)
        for block in (0, 2, 4):
            corrupt, alive = find_flips(base, block, want_alive=1)
            files += corrupt + alive
    assert sum(host_index(f)[2] == ACM_ERR_CORRUPT for f in files) == 12
    check(files, (INT16, BYTEPLANE, PACKED))


def test_truncation_at_every_byte():
    whole = make_stream(500, 5, 4, 3)
    assert len(whole) < 600 and host_index(whole)[1] == 3
    check([whole[:n] for n in range(len(whole) + 1)])


def test_truncation_of_a_stream_with_every_stager():
    """level 7, a few cuts per block: the byte-plane stager finds out that the file ends early only after it has written marks"""
    whole = make_stream(860, 7, 16, 6)
    marks = host_index(whole)[3]
    cuts = sorted({int(m["bit"]) // 8 + d for m in marks for d in (-1, 0, 1, 40)} | {len(whole) - 1})
    check([whole[:n] for n in cuts if 14 <= n < len(whole)], (INT16, BYTEPLANE, PACKED))


def test_short_files_and_not_acm():
    """0, 13, 14 and 19 bytes (nothing, a header one byte short - which the reader still takes -, a header and nothing, a header and a
    block's worth of bits), and a file that is not ACM: its marks buffer stays as poisoned"""
    whole = make_stream(870, 5, 4, 3)
    files = [whole[:0], whole[:13], whole[:14], whole[:19], b"RIFF this is not an acm file at all"]
    assert [host_index(f)[0] for f in files] == [-3, 0, 0, 0, -3]
    for f in (files[0], files[4]):
        for stager in (INT16, BYTEPLANE, PACKED):
            rc, info, raw = stage_marks(f, stager)
            assert rc == host_index(f)[0] and np.all(raw == POISON)
    check(files)
