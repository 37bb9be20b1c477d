"""Float32 PCM written by the synthesis kernels themselves (acmhip_plan_launch_f32, ACM_BATCH_PCM_F32, GpuDecoder(dtype=torch.float32))
on the GPU, against the CPU oracle.

A float sample is EXACTLY the ACMHIP_FMT_S16LE sample times 2^-15, so every comparison is an equality on bits.  Every kernel family a
plan can pick is forced in turn (plan flags, the byte-plane form bound); the float arena is poisoned with 0xFF bytes (NaN) before each
launch and guard floats around every stream must keep the poison; an int16 launch of the same plan gives the same PCM before and after a
float launch."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_stream, oracle_pcm, poison_pcm
from libacm_amd import capi

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats of poison between (and around) the streams of an arena: a multiple of 8


def f32_bits(s16):
    return (np.asarray(s16).view(np.int16).astype(np.float32) / np.float32(32768)).view(np.uint32)


def run_f32(dev, files, flags=capi.PLAN_AUTO, form="int16", windows=None):
    """one plan over `files`: int16 launch, float launch (arena poisoned), int16 launch again; every stream checked against the oracle,
    the guards around every stream still poisoned.  form: "int16" (the staged int16 rows) or "byteplane" (the byte-plane form bound)"""
    staged = [capi.stage_file(f) for f in files]
    ar = capi.Arena(staged, windows)
    n = len(staged)
    for k, d in enumerate(ar.descs):
        d.pcm_off += GUARD * (k + 1)            # poison in front of every stream and behind the last one
    words = ar.pcm_words + GUARD * (n + 1)
    d_idx, d_hdr = dev.malloc(ar.idx.nbytes), dev.malloc(ar.hdr.nbytes)
    d16, d32 = dev.malloc(words * 2), dev.malloc(words * 4)
    pk_ptrs = ()
    try:
        dev.upload(d_idx, ar.idx)
        dev.upload(d_hdr, ar.hdr)
        pk = None
        if form == "byteplane":
            # the form of the whole streams (a window into a stream reads its tiles from there: the lean kernels take a window that
            # starts on a tile boundary, behind a lead-in record for the tile in front of it)
            whole = capi.Arena(staged).descs
            for d, w in zip(whole, ar.descs):
                d.idx_off, d.hdr_off = w.idx_off, w.hdr_off
            pk = capi.mform_streams(ar.idx, whole)
            for p in ar.patch_list:
                pk.streams[p.stream].ntiles = 0
            pk_ptrs = pk.upload(dev)
        plan = capi.Plan(dev, ar.descs, ar.patches, flags, packed=pk.streams if pk else None)
        if pk:
            plan.bind_mform(*pk_ptrs)
        st = plan.stats()
        out16 = []
        for rep in range(2):
            dev.memset(d16, 0xA5, words * 2)
            plan.launch(d_idx, d_hdr, d16)
            h16 = np.empty(words, np.uint16)
            dev.download(h16, d16)
            out16.append(h16)
            if rep == 0:
                dev.memset(d32, 0xFF, words * 4)
                plan.launch_f32(d_idx, d_hdr, d32)
                h32 = np.empty(words, np.uint32)
                dev.download(h32, d32)
        dev.sync()
        plan.destroy()
    finally:
        for p in (d_idx, d_hdr, d16, d32) + tuple(pk_ptrs):
            dev.free(p)
    assert np.array_equal(out16[0], out16[1]), "an int16 launch after a float launch of the same plan differs"
    written = np.zeros(words, bool)
    for k, (f, s, d) in enumerate(zip(files, staged, ar.descs)):
        want, _ = oracle_pcm(f)
        rb = windows[k][0] if windows else 0
        want = want[(rb << s.info.level):(rb << s.info.level) + d.n_emit]
        a, b = d.pcm_off, d.pcm_off + d.n_emit
        assert np.array_equal(out16[0][a:b], want), ("int16", k)
        bad = np.nonzero(h32[a:b] != f32_bits(want))[0]
        assert bad.size == 0, "stream %d (level %d rows %d): %d of %d floats differ, first at %d" % (k, s.info.level, s.info.rows, bad.size, d.n_emit, bad[0])
        written[a:b] = True
    assert (h32[~written] == 0xFFFFFFFF).all(), "float writes outside the streams' samples: %s" % np.nonzero(h32[~written] != 0xFFFFFFFF)[0][:8]
    for rep in range(2):
        assert (out16[rep][~written] == 0xA5A5).all(), "int16 launch %d writes outside the streams' samples: %s" % (
            rep, np.nonzero(~written & (out16[rep] != 0xA5A5))[0][:8])
    return st


def window(f, frac, shorten=0):
    """(row_begin, n_emit) of a window from row nrows * frac on to the end of the stream's samples, `shorten` samples short of it"""
    s = capi.stage_file(f)
    nr = s.info.blocks * s.info.rows
    rb = min(nr - 1, int(nr * frac))
    return rb, max(1, s.words - (rb << s.info.level) - shorten)


# ---- every kernel family -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", list(range(16)))
def test_stagewise_every_level(dev, level):
    """ACMHIP_PLAN_STAGEWISE: unpack + one launch per stage + the emit kernel's float build, levels 0-15, awkward heights, windows"""
    files = [make_stream(9000 + 16 * level + r, level, r, max(2, min(12, (1 << 15) // (r << level))), cut=5 if level else 1)
             for r in (1, 3, 16)]
    st = run_f32(dev, files, flags=capi.PLAN_STAGEWISE)
    assert st.stagewise_streams == 3
    run_f32(dev, files, flags=capi.PLAN_STAGEWISE, windows=[window(f, 0.3, 3) for f in files])


@pytest.mark.parametrize("flags", [capi.PLAN_NO_LEAN | capi.PLAN_FORCE_HALO, capi.PLAN_NO_LEAN | capi.PLAN_FORCE_CARRY])
@pytest.mark.parametrize("level", list(range(16)))
def test_general_kernels_every_level(dev, flags, level):
    """no lean kernel: acm_small_level (0-4), acm_fused_tile in its halo and carry builds (5-12), the prefix sweep + the plane build of the
    tile kernel (13-15); block heights 1, odd and 16, ragged ends, several tiles per stream; windows into the streams"""
    files = []
    for r in (1, 5, 16):
        tr = max(1, ((32768 if level >= 11 else 16384) >> level))
        nb = max(2, min((3 * tr + r - 1) // r + 1, (1 << 21 >> level) // r, 1600))
        files.append(make_stream(9300 + 16 * level + r, level, r, nb, cut=7 if level else 1, channels=1 + r % 2 if level >= 4 else 1))
    run_f32(dev, files, flags=flags)
    run_f32(dev, files, flags=flags, windows=[window(f, 1 / 3, 3) for f in files])


@pytest.mark.parametrize("level,rows,blocks", [(0, 4095, 3), (3, 4095, 2), (5, 4095, 3), (9, 4095, 2), (12, 4095, 2), (13, 4095, 2)])
def test_rows_4095(dev, level, rows, blocks):
    """the tallest blocks acm_rows allows, on the general kernels and the lean ones"""
    f = make_stream(9600 + level, level, rows, blocks, cut=9)
    run_f32(dev, [f])
    run_f32(dev, [f], flags=capi.PLAN_LEAN_ALWAYS)


@pytest.mark.parametrize("level", list(range(6, 15)))
def test_lean_int16_form(dev, level):
    """ACMHIP_PLAN_LEAN_ALWAYS on the int16 form: acm_f32_tile2 takes the whole tiles (runs that start inside streams replay a lead-in
    tile into the sink), the general kernels the ragged tails; many streams, heights 1 / odd / 16 / 64"""
    files = []
    tr = (32768 >> level) if level >= 13 else (16384 >> level) if level >= 11 else (8192 >> level)
    for i, r in enumerate((1, 3, 16, 17, 64)):
        nb = max(2, (5 * max(tr, 1) + r - 1) // r + 1 + i)
        nb = min(nb, max(2, (1 << 22 >> level) // r))
        files.append(make_stream(9700 + 16 * level + r, level, r, nb, cut=5, channels=1 + i % 2,
                                 val_max=65535 if i % 2 else 255, pwr_max=15 if i % 2 else 12))
    st = run_f32(dev, files, flags=capi.PLAN_LEAN_ALWAYS)
    assert st.tiles >= 5
    run_f32(dev, files, flags=capi.PLAN_LEAN_ALWAYS, windows=[window(f, 0.5) for f in files])


@pytest.mark.parametrize("level", list(range(7, 15)))
def test_lean_byteplane_form(dev, level):
    """the byte-plane form bound: acm_f32_chunk (levels 8-12) and the matrix builds of acm_f32_tile2 (7, 13, 14); the 12-bit, 16-bit and
    whole-range width classes (small / large indices, 16-bit row values); windows whose lead-in chunks replay the rows in front"""
    files = []
    for i, (r, pmin, pmax, vmax) in enumerate(((16, 0, 3, 255), (3, 10, 12, 4095), (1, 13, 15, 65535), (17, 15, 15, 65535), (64, 0, 15, 65535))):
        tr = max(2, (16384 >> level))
        nb = max(2, min((4 * tr + r - 1) // r + 2, (1 << 22 >> level) // r + 1))
        files.append(make_stream(9800 + 16 * level + i, level, r, nb, cut=3 * i + 1, channels=1 + i % 2, pwr_min=pmin, pwr_max=pmax, val_max=vmax))
    st = run_f32(dev, files, flags=capi.PLAN_LEAN_ALWAYS, form="byteplane")
    assert st.mform_tiles > 0
    t2 = capi.lib().acmk_tile2_rows(level)
    w = []
    for f in files:
        s = capi.stage_file(f)
        rb = 2 * t2 if 3 * t2 <= s.info.blocks * s.info.rows else 0
        w.append((rb, s.words - (rb << level) - 1))
    st = run_f32(dev, files, flags=capi.PLAN_LEAN_ALWAYS, form="byteplane", windows=w)
    assert st.mform_tiles > 0 or level > 12            # (levels 13 / 14 leave the lean kernels to whole-stream plans)


def h1_streams(level, n, seed0):
    out = []
    for seed in range(seed0, seed0 + 60):
        f = make_stream(seed, level, 8, 30, pwr_min=0, pwr_max=3, mix=1)
        s = capi.stage_file(f)
        if s.patches is not None and len(s.patches):
            out.append(f)
            if len(out) == n:
                break
    assert len(out) == n
    return out


@pytest.mark.parametrize("form", ["int16", "byteplane"])
def test_h1_streams(dev, form):
    """hazard H1 (indices outside the block's table, resolved by the host parser as patches): the stage-wise path for the tiles that see
    a patch, the other kernels for the rest, next to clean streams"""
    files = h1_streams(6, 2, 9900) + h1_streams(8, 1, 9960) + [make_stream(9990, 9, 16, 40, cut=3)]
    run_f32(dev, files, form=form, flags=capi.PLAN_LEAN_ALWAYS)
    run_f32(dev, files)


def test_packed_form_is_refused(dev):
    """the packed staged form has no float build: a bound packed arena makes launch_f32 raise (and leaves the int16 launch alone)"""
    f = make_stream(9995, 9, 16, 24)
    s = capi.stage_file(f)
    ar = capi.Arena([s])
    pk = capi.pack_streams(ar.idx, ar.descs)
    ptrs = pk.upload(dev)
    d_idx, d_hdr, d_pcm = dev.malloc(ar.idx.nbytes), dev.malloc(ar.hdr.nbytes), dev.malloc(ar.pcm_words * 4)
    try:
        dev.upload(d_idx, ar.idx)
        dev.upload(d_hdr, ar.hdr)
        plan = capi.Plan(dev, ar.descs, None, capi.PLAN_LEAN_ALWAYS, packed=pk.streams)
        plan.bind_packed(*ptrs)
        with pytest.raises(capi.AcmHipError):
            plan.launch_f32(d_idx, d_hdr, d_pcm)
        assert "packed" in capi.lib().acmhip_last_error().decode()
        poison_pcm(dev, d_pcm, ar.pcm_words)
        plan.launch(d_idx, d_hdr, d_pcm)
        h = np.empty(ar.pcm_words, np.uint16)
        dev.download(h, d_pcm)
        assert np.array_equal(h[:ar.descs[0].n_emit], oracle_pcm(f)[0])
        plan.bind_packed(None, None)            # unbound: the float launch runs
        poison_pcm(dev, d_pcm, ar.pcm_words, f32=True)
        plan.launch_f32(d_idx, d_hdr, d_pcm)
        h32 = np.empty(ar.pcm_words, np.uint32)
        dev.download(h32, d_pcm)
        assert np.array_equal(h32[:ar.descs[0].n_emit], f32_bits(oracle_pcm(f)[0]))
        plan.destroy()
    finally:
        for p in (d_idx, d_hdr, d_pcm) + tuple(ptrs):
            dev.free(p)


# ---- the batch front end ------------------------------------------------------------------------------------------------------------

def batch_corpus():
    files = []
    for i in range(30):
        lv = 7 + i % 3
        rows = [16, 5, 1, 33][i % 4]
        files.append(make_stream(10000 + i, lv, rows, 2 + (i * 7) % 13 + (8192 >> lv) * (1 + i % 3) // rows, channels=1 + i % 2, cut=i % 5))
    files += h1_streams(7, 1, 10100)
    files.append(files[4][:len(files[4]) * 2 // 3])     # truncated
    files.append(b"not an acm file")
    return files


@pytest.mark.parametrize("parse,ranges", [(capi.PARSE_HOST, 0), (capi.PARSE_DEVICE, 1), (capi.PARSE_DEVICE, 3), (capi.PARSE_DEVICE, 16)])
@pytest.mark.parametrize("staging", [0, capi.BATCH_STAGE_INT16])
def test_batch_f32(dev, parse, ranges, staging):
    """ACM_BATCH_PCM_F32: statuses, words and dev_off those of the int16 call, the PCM that PCM / 32768 in bits, the padding between
    streams untouched (host parsing, device parsing in 1, 3 and 16 block ranges; byte-plane and int16 staging)"""
    files = batch_corpus()
    cap = capi.batch_pcm_words(files)
    d16, d32 = dev.malloc(cap * 2), dev.malloc(cap * 4)
    try:
        flags = staging | (capi.batch_ranges(ranges) if ranges else 0)
        dev.memset(d16, 0xA5, cap * 2)
        s16, w16, o16, _ = capi.batch_decode_device(dev, files, d16, cap, threads=4, parse=parse, batch_flags=flags)
        dev.memset(d32, 0xFF, cap * 4)
        s32, w32, o32, tm = capi.batch_decode_device(dev, files, d32, cap, threads=4, parse=parse, batch_flags=flags, f32=True)
        h16, h32 = np.empty(cap, np.uint16), np.empty(cap, np.uint32)
        dev.download(h16, d16)
        dev.download(h32, d32)
        dev.sync()
    finally:
        dev.free(d16)
        dev.free(d32)
    assert (s16, w16, o16) == (s32, w32, o32)
    assert s16[-1] != 0 and sum(1 for x in s16 if x == 0) >= 30
    if parse == capi.PARSE_DEVICE:
        assert tm.device_parsed > 0
    written = np.zeros(cap, bool)
    for k, f in enumerate(files):
        a, b = o16[k], o16[k] + w16[k]
        assert np.array_equal(h32[a:b], f32_bits(h16[a:b])), k
        written[a:b] = True
        if s16[k] == 0:
            assert np.array_equal(h16[a:b], oracle_pcm(f)[0]), k
    assert (h32[~written] == 0xFFFFFFFF).all()
    assert (h16[~written] == 0xA5A5).all()


def test_batch_f32_refusals(dev):
    """without device-resident output, with another format, with the packed staging: ACMHIP_ERR_ARG"""
    files = batch_corpus()[:4]
    bufs, items = capi._batch_items(files)
    d32 = dev.malloc(capi.batch_pcm_words(files) * 4)
    try:
        for fmt, flags, d_pcm in ((capi.FMT_S16LE, capi.BATCH_PCM_F32, None), (capi.FMT_S16BE, capi.BATCH_PCM_F32, d32),
                                  (capi.FMT_U16BE, capi.BATCH_PCM_F32, d32), (capi.FMT_S16LE, capi.BATCH_PCM_F32 | capi.BATCH_STAGE_PACKED, d32)):
            opts = capi.BatchOpts(0, fmt, 2, 0, capi.PARSE_HOST, flags, d_pcm, 1 << 24)
            assert capi.lib().acm_batch_decode(dev.h, items, len(files), C.byref(opts), None) == capi.ERR_ARG, (fmt, flags)
    finally:
        dev.free(d32)


def test_gpu_decoder_float32(dev):
    """GpuDecoder(dtype=torch.float32): a float32 cuda tensor equal to the int16 decoder's output / 32768"""
    import torch
    from libacm_amd import batch
    files = batch_corpus()
    p16, o16, w16, s16 = batch.GpuDecoder(0)(files)
    p32, o32, w32, s32 = batch.GpuDecoder(0, dtype=torch.float32)(files)
    assert p32.dtype == torch.float32 and p32.is_cuda and (o16, w16, s16) == (o32, w32, s32)
    for o, w in zip(o16, w16):
        assert torch.equal(p32[o:o + w], p16[o:o + w].float() / 32768)
    with pytest.raises(ValueError):
        batch.GpuDecoder(0, dtype=torch.float32, fmt=capi.FMT_S16BE)


# ---- full size ----------------------------------------------------------------------------------------------------------------------

def full_size_f32(dev, b, threads):
    """one plan over a full-size staged batch, byte-plane form bound, then the int16 form: both arenas in torch memory, the float one
    poisoned whole; the float PCM equals the int16 PCM / 32768 in bits on every stream, and the rest of the arena keeps its poison"""
    import torch
    bufs = b.upload(dev)
    mf = capi.mform_streams(b.idx, b.descs, threads=threads)
    mf_ptrs = mf.upload(dev)
    i16 = torch.empty(b.pcm_words, dtype=torch.int16, device="cuda")
    f32 = torch.empty(b.pcm_words, dtype=torch.float32, device="cuda")
    mask = np.zeros(b.pcm_words, bool)
    for d in b.descs:
        mask[d.pcm_off:d.pcm_off + d.n_emit] = True
    inside = torch.from_numpy(mask).cuda()
    del mask
    try:
        plan = capi.Plan(dev, b.descs, packed=mf.streams)
        for bind in (mf_ptrs, (None, None)):
            plan.bind_mform(*bind)
            i16.fill_(0x5A5A)
            f32.view(torch.int32).fill_(-1)
            torch.cuda.synchronize()
            plan.launch(bufs[0], bufs[1], i16.data_ptr())
            plan.launch_f32(bufs[0], bufs[1], f32.data_ptr())
            dev.sync()
            want = torch.where(inside, (i16.float() * (2.0 ** -15)).view(torch.int32), torch.full_like(f32, 0).view(torch.int32) - 1)
            assert torch.equal(f32.view(torch.int32), want), bind[0] is not None
            del want
        plan.destroy()
    finally:
        for p in bufs + mf_ptrs:
            dev.free(p)


def test_full_size_config_1_f32(dev):
    """configs[1] at full size (1024 mono streams, level 7, 16 rows, 1000 blocks: 2.1 Gsamples) in float32"""
    from libacm_amd import workload
    threads = max(4, min(64, workload.usable_cpus()))
    b = workload.build_uniform(1024, 7, 16, 1000, threads=threads)
    full_size_f32(dev, b, threads)


def test_full_size_config_2_f32(dev):
    """configs[2] at full size (4000 files, mono / stereo, levels 7-9, ragged ends: 1.9 Gsamples) in float32"""
    from libacm_amd import workload
    threads = max(4, min(64, workload.usable_cpus()))
    b = workload.build_corpus(4000, threads=threads)
    assert len(b.descs) == 4000
    full_size_f32(dev, b, threads)
