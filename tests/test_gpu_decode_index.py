"""acm_batch_decode_indexed on the GPU: the block index as a by-product of the decode's own parse (libacm_amd/csrc/acm_batch.cpp;
acm_parse.hip: the marks acm_parse_scan_wave and acm_parse_scan store beside the block headers).

Each case is one call, and decode_index.decode_both asserts four things about it: the index is acm_index_file's item by item; PCM,
words, offsets and statuses are those of the plain acm_batch_decode of the same arguments; (device_parsed, host_parsed) are the plain
call's - a fallback to acm_index_file on everything would not hide a kernel that stores nothing, because the marks of a stream the
device took come from nowhere else -; and the poison behind marks[blocks] is intact.  Streams are a few KB except where length is the
point."""
import ctypes as C
import io

import numpy as np
import pytest

from decode_index import decode, decode_both, index_info, room
from helpers import make_stream
from libacm_amd import capi
from test_gpu_batch_index import ACM_ERR_CORRUPT, TERN_LIMIT, find_flips, host_index, single, tern_groups, with_symbol

pytestmark = pytest.mark.gpu

RANGES = [1, 3, 16]


def device_takes(f):
    """must the device walk of a decode keep this stream?  Clean to its last block, supported, no H1 patch"""
    return host_index(f)[5] and index_info(f).npatches == 0


@pytest.fixture(scope="module")
def mixed():
    """a dozen streams: levels 5, 8, 9, 12, 13; rows 1, 3, 16, 255; blocks 1, 2, 7, 65, 300 - with 3 and 16 ranges the cuts are uneven and
    some ranges hold no block of the short streams; mono and stereo, one WAVC stream"""
    shapes = [(5, 16, 300, 1), (5, 255, 7, 1), (8, 3, 65, 1), (8, 16, 1, 2), (9, 16, 7, 1), (9, 255, 2, 1), (9, 1, 300, 1), (9, 3, 65, 2),
              (12, 3, 7, 1), (12, 1, 65, 1), (13, 1, 2, 1), (13, 3, 1, 2)]
    files = [make_stream(900 + i, lv, rows, nb, channels=ch, cut=(i % 3) * 7, wavc=1 if i == 7 else 0) for i, (lv, rows, nb, ch) in enumerate(shapes)]
    assert capi.probe(files[7])[1].header_bytes == 42
    return files


@pytest.mark.parametrize("ranges", RANGES)
def test_device_walk_whole_and_in_ranges(dev, mixed, ranges):
    got, plain = decode_both(dev, mixed, parse=capi.PARSE_DEVICE, batch_flags=capi.batch_ranges(ranges))
    want = sum(device_takes(f) for f in mixed)
    assert want == len(mixed) and got.device_parsed == want > 0 and got.host_parsed == 0


@pytest.fixture(scope="module")
def dirty():
    """dirty streams beside clean ones (level 5: ranges are cut at any block)"""
    L = capi.lib()
    clean = [make_stream(930 + i, 5, 8, 9) for i in range(4)]
    whole = make_stream(940, 5, 8, 9)
    marks = host_index(whole)[3]
    truncated = whole[:len(whole) * 3 // 4]
    # cut inside a block that lies in range 1 of 3 of what is left of the stream
    inside = whole[:(int(marks[4]["bit"]) + int(marks[5]["bit"])) // 16]
    b, done = room(inside), host_index(inside)[1]
    L.acmk_range_bound.restype = C.c_uint32
    L.acmk_range_bound.argtypes = [C.c_uint32] * 4
    assert L.acmk_range_bound(b, 1, 3, 1) <= done < L.acmk_range_bound(b, 2, 3, 1), (b, done)
    code, rows = 22, 17
    base = single(code, 7, rows, nblocks=3, seed=8)
    bad_symbol = with_symbol(base, code, 7, rows, 2, 127, tern_groups(code, rows) - 1, TERN_LIMIT[code])
    bad_code = find_flips(single(3, 5, 5, nblocks=5, seed=7), 2)[0][0]
    h1 = make_stream(950, 7, 16, 6, allow_out_of_range=1, pwr_min=0, pwr_max=3)
    assert index_info(h1).npatches > 0
    files = [clean[0], truncated, clean[1], inside, bad_symbol, base, bad_code, clean[2], h1, b"these bytes are not ACM", b"", clean[3]]
    assert [host_index(f)[2] for f in (bad_symbol, bad_code)] == [ACM_ERR_CORRUPT] * 2
    return files


@pytest.mark.parametrize("ranges", [1, 3])
def test_dirty_beside_clean(dev, dirty, ranges):
    """the dirty streams' marks come from the host reader's redo, the clean neighbours' from the device"""
    got, plain = decode_both(dev, dirty, parse=capi.PARSE_DEVICE, batch_flags=capi.batch_ranges(ranges))
    want = sum(device_takes(f) for f in dirty)
    assert want == 5 and got.device_parsed == want and got.host_parsed == 5


def test_lane_per_stream_walk(dev):
    """more streams than the wave-per-stream walk takes: acm_parse_scan stores the marks from its lanes and reports where it ended.  The
    population of tests/test_gpu_parity.py::test_device_walk_lane_kernel"""
    files = [make_stream(9100 + i % 97, 3 + i % 2, 2, 1 + i % 2, cut=i % 3) for i in range(33000)]
    got, plain = decode_both(dev, files, parse=capi.PARSE_DEVICE, threads=8)
    assert got.device_parsed >= 32900


@pytest.fixture(scope="module")
def host_batch(mixed, dirty):
    return mixed[2:6] + dirty + [make_stream(960, 7, 16, 12), make_stream(961, 9, 8, 16, cut=100)]


@pytest.mark.parametrize("stage", ["byteplane", "int16", "packed", "prestaged"])
def test_host_pool(dev, host_batch, stage):
    flags = {"byteplane": capi.BATCH_STAGE_BYTEPLANE, "int16": capi.BATCH_STAGE_INT16, "packed": capi.BATCH_STAGE_PACKED, "prestaged": 0}[stage]
    got, plain = decode_both(dev, host_batch, parse=capi.PARSE_HOST, batch_flags=flags, prestage=stage == "prestaged")
    assert got.device_parsed == 0 and got.host_parsed == sum(host_index(f)[0] == 0 for f in host_batch)


@pytest.mark.parametrize("where", ["host", "device_s16", "device_f32"])
@pytest.mark.parametrize("parse", [capi.PARSE_DEVICE, capi.PARSE_HOST])
def test_index_does_not_depend_on_where_the_pcm_goes(dev, mixed, dirty, parse, where):
    files = mixed[3:8] + dirty
    decode_both(dev, files, parse=parse, device_out=where != "host", f32=where == "device_f32")


def test_no_room_for_the_index(dev, mixed):
    """ACMHIP_ERR_ARG before any work is done: items and a poisoned PCM buffer stay as they are"""
    files = mixed[:3] + [b"not ACM"]
    for kw in ({"short": 1}, {"null_marks": 2}):
        r = decode(dev, files, True, parse=capi.PARSE_DEVICE, **kw)
        assert r.rc == capi.ERR_ARG
        assert r.statuses == [0] * 4 and r.words == [0] * 4 and r.offs == [0] * 4
        assert all(np.all(p == 0x5A5A) for p in r.pcm) and all(np.all(m == 0xA5) for m in r.marks)
        assert r.ix == [(77, 77, 77)] * 4
    # room for a file that is not ACM is nobody's concern
    r = decode(dev, files, True, parse=capi.PARSE_DEVICE, null_marks=3)
    assert r.rc == 0 and r.ix[3][1:] == (0, 0) and r.ix[3][0] != 0


def test_second_call_on_the_same_handle(mixed, dirty):
    """the marks arenas are reused: a smaller batch after a larger one, other files in the same slots"""
    with capi.Device(0) as d2:
        for parse in (capi.PARSE_DEVICE, capi.PARSE_HOST):
            decode_both(d2, mixed, parse=parse)
            decode_both(d2, dirty[::-1], parse=parse)
            decode_both(d2, [mixed[4]], parse=parse)
            decode_both(d2, [b"junk", b""], parse=parse)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_decode_then_crop(dtype):
    """dec(files, return_index=True), then dec.crop(files, windows, index): every crop is the slice of the whole decode just returned"""
    import torch
    from libacm_amd import batch
    files = [make_stream(970 + i, lv, rows, 5, cut=11) for i, (lv, rows) in enumerate(((5, 16), (8, 16), (9, 3), (11, 4)))] + [b"no acm"]
    dec = batch.GpuDecoder(0, parse=capi.PARSE_DEVICE, dtype=getattr(torch, dtype))
    try:
        assert len(dec(files)) == 4
        pcm, offs, counts, statuses, index = dec(files, return_index=True)
        whole = pcm.cpu().numpy().copy()
        assert dec.timing.device_parsed == 4
        for f, ix in zip(files, index):
            rc, blocks, end, marks, promised, s = host_index(f)
            assert isinstance(ix, capi.BlockIndex) and np.array_equal(np.asarray(ix), marks) and ix.end_status == (end if rc == 0 else None)
        # the index survives np.save / np.load
        kept = []
        for ix in index:
            buf = io.BytesIO()
            np.save(buf, np.asarray(ix))
            buf.seek(0)
            kept.append(np.load(buf))
            assert kept[-1].dtype == capi.BLOCK_MARK_DT and np.array_equal(kept[-1], np.asarray(ix))
        windows = []
        for k in range(4):
            bl = index_info(files[k]).rows * index_info(files[k]).cols
            windows += [(k, 0, 100), (k, bl - 37, 90), (k, 2 * bl + 5, bl), (k, counts[k] - 50, 200)]       # start, block border, ragged end
        windows.append((4, 0, 10))
        for ixs in (index, kept):
            out, o, n, st = dec.crop(files, windows, ixs)
            out = out.cpu().numpy()
            for w, (k, first, count) in enumerate(windows):
                want = whole[offs[k] + first:offs[k] + min(first + count, counts[k])] if k < 4 else whole[:0]
                assert n[w] == len(want) and np.array_equal(out[o[w]:o[w] + n[w]], want), (w, k, first, count)
    finally:
        dec.dev.close()
