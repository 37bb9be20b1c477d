"""acm_batch_index_files without a GPU (libacm_amd/csrc/acm_batch_index.cpp): the exported symbols, the host pool behind
ACM_BATCH_PARSE_HOST with no device handle, and the refusal of ACM_BATCH_PARSE_DEVICE without one.  The expected value is
capi.index_file, item by item - the host index the crop tests already trust."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_stream
from libacm_amd import batch, capi

ACM_ERR_NOT_ACM = -3


def host_index(data, max_blocks=None, force_chans=0):
    """acm_index_file itself -> (rc, blocks, end_status, marks[0 .. blocks])"""
    a = capi._as_u8(data)
    rc, info = capi.probe(a, force_chans)
    room = max_blocks
    if room is None:
        room = 0
        if rc == 0:
            bl = info.rows * info.cols
            room = min((info.total_values + bl - 1) // bl, (max(0, a.size - info.header_bytes) * 8 + 8) // (20 + 5 * info.cols) + 1)
    marks = np.zeros(room + 1, dtype=capi.BLOCK_MARK_DT)
    st = capi.StageInfo()
    rc = capi.lib().acm_index_file(a.ctypes.data, a.size, force_chans, marks.ctypes.data, room, C.byref(st))
    return rc, st.blocks, st.end_status, marks[:st.blocks + 1] if rc == 0 else marks[:0]


def mixed_files():
    files = [make_stream(40 + i, lv, rows, nb, cut=cut) for i, (lv, rows, nb, cut) in enumerate([(0, 5, 9, 2), (5, 8, 6, 0), (9, 16, 5, 77), (13, 2, 3, 0)])]
    files.append(make_stream(50, 7, 8, 4, wavc=1))
    files.append(b"RIFF this is not an ACM stream at all")
    files.append(b"")
    files.append(files[2][:len(files[2]) * 2 // 3])         # truncated inside a block
    files.append(files[1][:15])                             # a header and one byte
    return files


def test_new_symbols_are_exported():
    L = capi.lib()
    for name in ("acm_batch_index_files", "acm_batch_index_blocks", "acmk_launch_index", "acmk_index_layout_visit"):
        assert hasattr(L, name), name
    assert "acm_batch_index_files" in capi.ACMHIP_SYMBOLS and "acm_batch_index_blocks" in capi.ACMHIP_SYMBOLS


@pytest.mark.parametrize("threads", [1, 4])
def test_host_pool_without_a_device_equals_index_file(threads):
    files = mixed_files()
    got, tm, status = capi.batch_index_files(None, files, parse=capi.PARSE_HOST, threads=threads, return_status=True)
    assert len(got) == len(files)
    for i, f in enumerate(files):
        rc, blocks, end, marks = host_index(f)
        assert status[i] == rc, i
        if rc != 0:
            assert rc == ACM_ERR_NOT_ACM and len(got[i]) == 0
            continue
        assert len(got[i]) == blocks + 1 and got[i].end_status == end, (i, len(got[i]), blocks, got[i].end_status, end)
        assert np.array_equal(np.asarray(got[i]), marks), i
    assert (tm.host_indexed, tm.device_indexed, tm.groups) == (len(files), 0, 0)
    assert tm.blocks == sum(len(g) - 1 for g in got if len(g))
    # the truncated file is a case: fewer blocks than promised, and a reason
    assert len(got[7]) - 1 < len(got[2]) - 1 and (got[7].end_status != 0 or len(got[7]) - 1 < 5)


def test_too_small_max_blocks():
    files = mixed_files()[:5]
    for room in (0, 1, 2):
        got, tm, status = capi.batch_index_files(None, files, parse=capi.PARSE_HOST, max_blocks=room, return_status=True)
        for i, f in enumerate(files):
            rc, blocks, end, marks = host_index(f, max_blocks=room)
            assert (status[i], len(got[i]) - 1, got[i].end_status) == (rc, blocks, end) and blocks == room
            assert np.array_equal(np.asarray(got[i]), marks), (room, i)


def test_capacity_call():
    files = mixed_files()
    bufs, items = capi._batch_items(files)
    per = np.zeros(len(files), dtype=np.uint64)
    total = capi.lib().acm_batch_index_blocks(items, len(files), 0, per.ctypes.data)
    assert total == per.sum()
    for i, f in enumerate(files):
        rc, blocks, end, marks = host_index(f)
        assert per[i] >= blocks and (rc == 0 or per[i] == 0)
    assert capi.lib().acm_batch_index_blocks(items, len(files), 0, None) == total


def test_device_parse_needs_a_device():
    files = mixed_files()[:2]
    bufs, items = capi._batch_items(files)
    out = (capi.BatchIndexOut * 2)()
    opts = capi.IndexOpts(0, 1, capi.PARSE_DEVICE, 0, 0)
    assert capi.lib().acm_batch_index_files(None, items, 2, out, C.byref(opts), None) == capi.ERR_NO_DEVICE
    opts.parse = 3
    assert capi.lib().acm_batch_index_files(None, items, 2, out, C.byref(opts), None) == capi.ERR_ARG
    # AUTO without a device is the pool
    got, tm = capi.batch_index_files(None, files, parse=capi.PARSE_AUTO)
    assert tm.host_indexed == 2 and all(np.array_equal(np.asarray(g), np.asarray(capi.index_file(f)[0])) for g, f in zip(got, files))


def test_build_index_keeps_its_default():
    """batch.build_index(files) without a decoder is the host parser, file by file, as before"""
    files = mixed_files()
    got = batch.build_index(files, threads=2)
    for i, f in enumerate(files):
        rc, blocks, end, marks = host_index(f)
        assert np.array_equal(np.asarray(got[i]), marks), i
        if rc == 0:
            assert got[i].end_status == end
