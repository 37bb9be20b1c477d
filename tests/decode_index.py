"""Shared by tests/test_decode_index.py and tests/test_gpu_decode_index.py: the block index as a by-product of whoever parses a stream
for acm_batch_decode (include/acm_hip.h: acm_batch_decode_indexed, acm_batch_prestaged_index; the test hook acmk_stage_marks).

Every expectation here is the host's acm_index_file (host_index of tests/test_gpu_batch_index.py, computed once per file image) - never
the path under test.  Marks buffers are handed over full of POISON bytes with PAD entries more than the call may write, so that a
store behind marks[blocks] shows."""
import ctypes as C

import numpy as np

from libacm_amd import capi
from test_gpu_batch_index import host_index

POISON = 0xA5
PAD = 3                 # entries behind the B + 1 a call may write
PCM_POISON = 0x5A5A

INT16, BYTEPLANE, PACKED = 0, 1, 2      # acmk_stage_marks: the stager


def room(data):
    """B of the issue: the per-item value of acm_batch_index_blocks (0 for a file that is not ACM)"""
    bufs, items = capi._batch_items([data])
    per = np.zeros(1, dtype=np.uint64)
    capi.lib().acm_batch_index_blocks(items, 1, 0, per.ctypes.data)
    return int(per[0])


def poisoned(entries):
    return np.full(entries * capi.BLOCK_MARK_DT.itemsize, POISON, dtype=np.uint8)


def expect_marks(raw, data, what):
    """raw: the bytes of a marks buffer that was all POISON.  It must hold acm_index_file's marks[0 .. blocks] and poison behind them -
    all poison for a file that is not ACM.  Returns the host's (rc, blocks, end_status)"""
    rc, blocks, end, marks, promised, s = host_index(data)
    got = raw.view(capi.BLOCK_MARK_DT)
    used = blocks + 1 if rc == 0 else 0
    assert np.array_equal(got[:used], marks), (what, got[:used], marks)
    assert np.all(raw[used * capi.BLOCK_MARK_DT.itemsize:] == POISON), (what, "poison behind marks[blocks] overwritten")
    return rc, blocks, end


def stagers_of(level):
    """the host stagers a batch's pool can pick at this level"""
    L = capi.lib()
    return [INT16] + ([BYTEPLANE] if L.acmhip_mform_tile_rows(level) > 0 else []) + ([PACKED] if L.acmhip_packed_tile_rows(level) > 0 else [])


def stage_marks(data, stager):
    """acmk_stage_marks -> (rc, StageInfo, raw bytes of the poisoned marks buffer)"""
    fn = capi.lib().acmk_stage_marks
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(capi.StageInfo)]
    a = capi._as_u8(data)
    b = room(data)
    raw = poisoned(b + 1 + PAD)
    info = capi.StageInfo()
    rc = fn(a.ctypes.data, a.size, 0, stager, raw.ctypes.data, b, C.byref(info))
    return rc, info, raw


def check_hook(files, levels_with=()):
    """every file through every stager its level has: (rc, info, marks) are acm_index_file's"""
    seen = set()
    for k, f in enumerate(files):
        prc, pinfo = capi.probe(f)
        for stager in (stagers_of(pinfo.level) if prc == 0 else [INT16, BYTEPLANE, PACKED]):
            rc, info, raw = stage_marks(f, stager)
            want = expect_marks(raw, f, (k, stager))
            assert rc == want[0], (k, stager, rc, want)
            if rc == 0:
                assert (info.blocks, info.end_status) == want[1:], (k, stager, info.blocks, info.end_status, want)
                assert info.npatches == index_info(f).npatches, (k, stager)
                seen.add(stager)
    for stager in levels_with:
        assert stager in seen, ("no file reached stager", stager)


_info = {}


def index_info(data):
    data = bytes(data)
    if data not in _info:
        a = capi._as_u8(data)
        b = room(data)
        marks = np.zeros(b + 1, dtype=capi.BLOCK_MARK_DT)
        st = capi.StageInfo()
        assert capi.lib().acm_index_file(a.ctypes.data, a.size, 0, marks.ctypes.data, b, C.byref(st)) == 0
        _info[data] = st
    return _info[data]


def check_prestage(files, threads=2):
    """acm_batch_prestage keeps the marks of what it parses; acm_batch_prestaged_index hands out acm_index_file's answer"""
    L = capi.lib()
    bufs, items = capi._batch_items(files)
    n = len(files)
    opts = capi.BatchOpts(0, capi.FMT_S16LE, threads, 0, capi.PARSE_HOST, 0)
    pre = C.c_void_p()
    assert L.acm_batch_prestage(items, n, C.byref(opts), C.byref(pre), None) == 0
    try:
        for k, f in enumerate(files):
            rc, blocks, end, marks, promised, s = host_index(f)
            mp, nb, es = C.c_void_p(), C.c_uint32(123), C.c_int32(123)
            got = L.acm_batch_prestaged_index(pre, k, C.byref(mp), C.byref(nb), C.byref(es))
            assert got == rc, (k, got, rc)
            if rc != 0:
                assert not mp.value and (nb.value, es.value) == (0, 0), k
                continue
            assert (nb.value, es.value) == (blocks, end), (k, nb.value, es.value, blocks, end)
            view = np.ctypeslib.as_array(C.cast(mp, C.POINTER(C.c_uint8)), shape=((blocks + 1) * capi.BLOCK_MARK_DT.itemsize,))
            assert np.array_equal(view.view(capi.BLOCK_MARK_DT), marks), k
        mp, nb, es = C.c_void_p(), C.c_uint32(), C.c_int32()
        assert L.acm_batch_prestaged_index(pre, n, C.byref(mp), C.byref(nb), C.byref(es)) == capi.ERR_ARG
    finally:
        L.acm_batch_prestage_free(pre)


# ---- one acm_batch_decode / acm_batch_decode_indexed call with everything it may write poisoned (GPU tests) -----------------------

class Call:
    pass


def decode(dev, files, indexed, parse=capi.PARSE_DEVICE, batch_flags=0, threads=4, prestage=False, device_out=False, f32=False,
           short=None, null_marks=None):
    """-> Call: rc, statuses, words, offs, pcm (host output: one poisoned array per item; device output: the whole poisoned buffer, read
    back), device_parsed, host_parsed, and with indexed=True marks[i] (raw bytes), ix[i] = (status, blocks, end_status).
    short / null_marks: the item whose max_blocks is one too small / whose marks are NULL"""
    L = capi.lib()
    n = len(files)
    bufs, items = capi._batch_items(files)
    r = Call()
    sizes = [i.total_values if rc == 0 else 0 for rc, i in (capi.probe(b) for b in bufs)]
    d_pcm, words = None, 0
    if device_out:
        words = int(L.acm_batch_pcm_words(items, n, 0))
        nbytes = max(words, 1) * (4 if f32 else 2)
        d_pcm = dev.malloc(nbytes)
        dev.memset(d_pcm, 0x5A, nbytes)
    else:
        r.pcm = [np.full(max(sz, 1), PCM_POISON, dtype=np.uint16) for sz in sizes]
        for k in range(n):
            items[k].pcm = r.pcm[k].ctypes.data if sizes[k] else None
            items[k].pcm_cap = sizes[k]
    opts = capi.BatchOpts(0, capi.FMT_S16LE, threads, 0, parse, batch_flags | (capi.BATCH_PCM_F32 if f32 else 0), d_pcm, words)
    tm = capi.BatchTiming()
    pre = C.c_void_p()
    try:
        if prestage:
            assert L.acm_batch_prestage(items, n, C.byref(opts), C.byref(pre), None) == 0
            opts.prestaged = pre
        if indexed:
            need = [room(f) for f in files]
            r.marks = [poisoned(b + 1 + PAD) for b in need]
            out = (capi.BatchIndexOut * max(n, 1))()
            for k in range(n):
                out[k].marks = None if k == null_marks else r.marks[k].ctypes.data
                out[k].max_blocks = need[k] - 1 if k == short else need[k]
                out[k].blocks, out[k].end_status, out[k].status = 77, 77, 77
            r.rc = L.acm_batch_decode_indexed(dev.h, items, n, C.byref(opts), out, C.byref(tm))
            r.ix = [(out[k].status, out[k].blocks, out[k].end_status) for k in range(n)]
        else:
            r.rc = L.acm_batch_decode(dev.h, items, n, C.byref(opts), C.byref(tm))
        if device_out:
            r.pcm = np.zeros(max(words, 1) * (2 if f32 else 1), dtype=np.uint16)
            dev.download(r.pcm, d_pcm)
    finally:
        if pre:
            L.acm_batch_prestage_free(pre)
        if d_pcm is not None:
            dev.free(d_pcm)
    r.statuses = [int(items[k].status) for k in range(n)]
    r.words = [int(items[k].words) for k in range(n)]
    r.offs = [int(items[k].dev_off) for k in range(n)]
    r.device_parsed, r.host_parsed = int(tm.device_parsed), int(tm.host_parsed)
    return r


def same_pcm(a, b):
    if isinstance(a.pcm, list):
        return all(np.array_equal(x, y) for x, y in zip(a.pcm, b.pcm))
    return np.array_equal(a.pcm, b.pcm)


def decode_both(dev, files, **kw):
    """the four assertions of every case: one indexed call against acm_index_file and against the plain call of the same arguments.
    -> (indexed Call, plain Call)"""
    plain = decode(dev, files, False, **kw)
    got = decode(dev, files, True, **kw)
    assert plain.rc == 0 and got.rc == 0, (plain.rc, got.rc, capi.lib().acmhip_last_error())
    # 1. the index is acm_index_file's, item by item; 4. poison behind marks[blocks] is intact
    for k, f in enumerate(files):
        rc, blocks, end = expect_marks(got.marks[k], f, k)
        assert got.ix[k] == (rc, blocks if rc == 0 else 0, end if rc == 0 else 0), (k, got.ix[k], rc, blocks, end)
    # 2. PCM, words and statuses are the plain call's
    assert (got.statuses, got.words, got.offs) == (plain.statuses, plain.words, plain.offs)
    assert same_pcm(got, plain)
    # 3. nobody parsed a stream who would not have parsed it anyway
    print("n %d  device_parsed %d  host_parsed %d  (plain: %d, %d)" % (len(files), got.device_parsed, got.host_parsed, plain.device_parsed, plain.host_parsed))
    assert (got.device_parsed, got.host_parsed) == (plain.device_parsed, plain.host_parsed)
    return got, plain
