"""acm_batch_decode_windows on the GPU: random-access crops through a block index (libacm_amd/csrc/acm_batch_windows.cpp,
acm_parse.hip: acm_parse_scan_blocks).

Expected PCM is the CPU oracle's whole-file decode, sliced; expected words / status / block ranges come from the pure-Python rule of
tests/test_block_index.py (expected_window).  Every call writes into a poisoned arena with guard bands: outside the slots the call
reports nothing may change, inside a slot [dev_off, dev_off + words) is the oracle's slice."""
import numpy as np
import pytest

from helpers import fmt_args, make_stream, oracle_pcm
from libacm_amd import capi
from test_block_index import expected_window

pytestmark = pytest.mark.gpu

GUARD = 512
POISON16, POISON32 = 0xA5A5, 0xA5A5A5A5
BOTH = (capi.PARSE_HOST, capi.PARSE_DEVICE)
ACM_ERR_NOT_ACM = -3


class Src:
    """a file, its index and what the host parser says about it"""

    def __init__(self, data, force_chans=0):
        self.data = data
        rc, _ = capi.probe(data, force_chans)
        self.st = capi.stage_file(data, force_chans) if rc == 0 else None
        self.rc = rc
        self.marks, self.ix = capi.index_file(data, force_chans) if rc == 0 else (None, None)
        self._pcm = {}

    def pcm(self, fmt=capi.FMT_S16LE, force_chans=0):
        if fmt not in self._pcm:
            be, sg = fmt_args(fmt)
            self._pcm[fmt] = oracle_pcm(self.data, force_chans, be, sg)[0]
        return self._pcm[fmt]

    def expect(self, first, count):
        return expected_window(self.st, self.rc, first, count)


def as_f32(u16):
    return (u16.view(np.int16).astype(np.float32) / np.float32(32768.0))


def run(dev, srcs, windows, parse, fmt=capi.FMT_S16LE, f32=False, index=None, check=True, threads=4, flags=capi.PLAN_AUTO):
    """one device-resident call into a poisoned arena -> (per-window arrays, statuses, words, slots, timing); checks the poison
    outside the slots, and (check=True) words, statuses, PCM and the block accounting against the oracle"""
    files = [s.data for s in srcs]
    index = [s.marks for s in srcs] if index is None else index
    cap = capi.batch_window_pcm_words(files, windows)
    unit, dt, poison = (4, np.uint32, POISON32) if f32 else (2, np.uint16, POISON16)
    total = cap + 2 * GUARD
    d = dev.malloc(total * unit)
    try:
        dev.memset(d, 0xA5, total * unit)
        st, words, offs, slots, tm = capi.batch_decode_windows_device(dev, files, index, windows, d + GUARD * unit, cap, fmt=fmt, parse=parse,
                                                                      f32=f32, threads=threads, flags=flags)
        raw = np.zeros(total, dtype=dt)
        dev.download(raw, d)
    finally:
        dev.free(d)
    untouched = np.ones(total, dtype=bool)
    end = 0
    for k, (so, sw) in enumerate(slots):
        assert so >= end and so % 8 == 0, (k, so, end)          # slots in order, never overlapping
        end = so + sw
        assert so <= offs[k] and offs[k] + words[k] <= so + sw, k
        untouched[GUARD + so:GUARD + so + sw] = False
    assert end <= cap
    assert np.all(raw[untouched] == poison), "the call wrote outside its slots"
    got = [raw[GUARD + offs[k]:GUARD + offs[k] + words[k]] for k in range(len(windows))]
    if check:
        nblocks = 0
        for k, (f, first, count) in enumerate(windows):
            w, status, b0, nb = srcs[f].expect(first, count)
            nblocks += nb
            assert (words[k], st[k]) == (w, status), (k, windows[k], words[k], st[k], w, status)
            want = srcs[f].pcm(fmt)[first:first + w]
            if f32:
                assert np.array_equal(got[k], as_f32(want).view(np.uint32)), (k, windows[k])
            else:
                assert np.array_equal(got[k], want), (k, windows[k])
        assert tm.blocks_parsed == nblocks              # the index is used: nothing in front of a window is parsed
        assert tm.samples == sum(words)
    return got, st, words, slots, tm


def window_kinds(src):
    """the ten kinds of window of the matrix, for one stream"""
    st = src.st
    W, bl, cols, nb = st.words, st.block_len, st.info.cols, st.info.blocks
    odd = next(v for v in range(cols + 1, cols + 40) if (cols == 1 or v % cols) and v % 8)
    return [(0, min(W, 100)),                           # from 0
            (min(1, cols - 1), max(1, cols // 2)),      # inside the first row
            (min(odd, W - 1), 77),                      # first_word a multiple of neither cols nor 8
            (max(bl - 2, 0), 5),                        # across a block boundary
            ((nb - 1) * bl, W - (nb - 1) * bl),         # the last, partial block
            (0, W),                                     # the whole file
            (max(W - 10, 0), 50),                       # reaching past the end
            (W + 5, 10),                                # starting behind the end
            (3, 0),                                     # zero length
            (W // 3, W // 3), (W // 3 + W // 6, W // 3)]        # two overlapping windows


def matrix_stream(level, rows, k=0):
    bl = rows << level
    nb = 3 if bl >= 4096 else min(40, 4096 // bl + 3)
    return make_stream(6100 + 16 * level + k, level, rows, nb, channels=1 + ((level + rows) % 2 if bl % 2 == 0 else 0), cut=max(1, bl // 3) if bl > 1 else 0, mix=level % 2)


def h2d_bound(srcs, windows, host_windows=()):
    """device parsing uploads the byte span of each window's blocks (from a dword boundary; padded to 16 bytes, 16 zero bytes behind),
    one 72-byte job record per window and one 24-byte record per block, each table padded to 64 bytes - and, for a window the host staged
    again, its int16 rows and block headers"""
    total, nwin, nblk = 0, 0, 0
    for k, (f, first, count) in enumerate(windows):
        w, status, b0, nb = srcs[f].expect(first, count)
        if not w:
            continue
        m = srcs[f].marks
        span = min(len(srcs[f].data), (int(m["bit"][b0 + nb]) + 7) // 8) - (int(m["bit"][b0]) // 8 & ~3)
        total += (span + 15) // 16 * 16 + 16
        nwin += 1
        nblk += nb
        if k in host_windows:
            total += nb * srcs[f].st.block_len * 2 + nb * 8
    return total + (72 * nwin + 63) // 64 * 64 + (24 * nblk + 63) // 64 * 64


@pytest.mark.parametrize("level", range(16))
def test_window_matrix(dev, level):
    srcs = [Src(matrix_stream(level, rows)) for rows in (1, 3, 16, 255)]
    windows = [(f, a, n) for f, s in enumerate(srcs) for a, n in window_kinds(s)]
    for parse in BOTH:
        got, st, words, slots, tm = run(dev, srcs, windows, parse)
        if parse == capi.PARSE_DEVICE:
            assert tm.host_parsed == 0 and tm.device_parsed == sum(1 for w in words if w)
            assert tm.h2d_bytes <= h2d_bound(srcs, windows)
        else:
            assert tm.device_parsed == 0 and tm.host_parsed == sum(1 for w in words if w)


@pytest.mark.parametrize("fmt", [capi.FMT_S16LE, capi.FMT_S16BE, capi.FMT_U16LE, capi.FMT_U16BE])
def test_formats_and_host_output(dev, fmt):
    srcs = [Src(matrix_stream(lv, rows, 1)) for lv, rows in ((3, 5), (5, 16), (7, 3), (9, 16), (11, 2), (13, 1))]
    windows = [(f, a, n) for f, s in enumerate(srcs) for a, n in window_kinds(s)]
    files, index = [s.data for s in srcs], [s.marks for s in srcs]
    for parse in BOTH:
        run(dev, srcs, windows, parse, fmt=fmt)
        # host output; every third buffer smaller than its window
        caps = [n if k % 3 else n // 2 for k, (f, a, n) in enumerate(windows)]
        res, tm = capi.batch_decode_windows(dev, files, index, windows, fmt=fmt, parse=parse, threads=3, caps=caps)
        for k, (f, a, n) in enumerate(windows):
            w, status, b0, nb = srcs[f].expect(a, n)
            assert (res[k][0], res[k][1]) == (status, w), (k, windows[k])
            assert np.array_equal(res[k][2], srcs[f].pcm(fmt)[a:a + min(w, caps[k])]), (k, windows[k])


def test_float32_output(dev):
    srcs = [Src(matrix_stream(lv, rows, 2)) for lv, rows in ((0, 16), (4, 3), (6, 16), (9, 16), (12, 3), (14, 1))]
    windows = [(f, a, n) for f, s in enumerate(srcs) for a, n in window_kinds(s)]
    for parse in BOTH:
        run(dev, srcs, windows, parse, f32=True)
    files, index = [s.data for s in srcs], [s.marks for s in srcs]
    with pytest.raises(capi.AcmHipError):               # float32 samples are device-resident only
        bufs, items, ix, wins, keep = capi._window_tables(files, index, windows)
        opts = capi.BatchOpts(0, capi.FMT_S16LE, 0, 0, capi.PARSE_HOST, capi.BATCH_PCM_F32)
        capi._check(capi.lib().acm_batch_decode_windows(dev.h, items, len(files), ix, wins, len(windows), opts, None), "windows")
    for flags in (capi.BATCH_STAGE_PACKED,):            # forms a window does not have
        bufs, items, ix, wins, keep = capi._window_tables(files, index, windows)
        opts = capi.BatchOpts(0, capi.FMT_S16LE, 0, 0, capi.PARSE_HOST, flags)
        assert capi.lib().acm_batch_decode_windows(dev.h, items, len(files), ix, wins, len(windows), opts, None) == capi.ERR_ARG
    d = dev.malloc(1 << 16)
    with pytest.raises(capi.AcmHipError):               # too small a buffer is refused
        capi.batch_decode_windows_device(dev, files, index, windows, d, 64)
    dev.free(d)


def h1_sources():
    return [Src(make_stream(900 + lv, lv, rows, 8, mix=1, allow_out_of_range=1, prime_table=1, pwr_min=0, pwr_max=6))
            for lv, rows in ((3, 4), (5, 16), (7, 16), (9, 4))] + \
           [Src(make_stream(800 + seed, 5, 7, 8, mix=1, allow_out_of_range=1, prime_table=1, pwr_min=0, pwr_max=15, val_min=0, val_max=65535))
            for seed in range(4)]


def test_h1_streams(dev):
    """stale-table reads: the host stager patches them from the marks' history; the device parser flags the window and the host
    stages it again"""
    srcs = h1_sources() + [Src(matrix_stream(6, 16, 3))]
    assert all(s.st.info.npatches > 0 for s in srcs[:-1])
    windows = [(f, a, n) for f, s in enumerate(srcs) for a, n in window_kinds(s)]
    windows += [(f, b * s.st.block_len + 7, s.st.block_len) for f, s in enumerate(srcs[:-1]) for b in range(1, 7)]
    run(dev, srcs, windows, capi.PARSE_HOST)
    got, st, words, slots, tm = run(dev, srcs, windows, capi.PARSE_DEVICE)
    assert tm.host_parsed > 0 and tm.device_parsed > 0
    assert tm.device_parsed + tm.host_parsed == sum(1 for w in words if w)


SINGLE_CODES = (17, 18, 20, 21, 23, 24, 26, 27) + (19, 22, 29)         # the eight k-fillers, the three ternary ones
SINGLE_ROWS = (1, 2, 15, 16, 17, 31, 40, 255)                           # around the 16-row switch of the jump table, one row, tall columns
SINGLE_LEVELS = (3, 5, 6, 7)                                            # 8, 32, 64, 128 columns: below, at and above one wavefront's 64 offsets


def single_filler_sources():
    """(srcs, windows): three-block streams of ONE filler each, every one whole and clean for the host reader (asserted here, without
    a device); per stream the whole file and a window that starts inside the last block"""
    from libacm_amd import synth
    srcs, windows = [], []
    for code in SINGLE_CODES:
        for rows in SINGLE_ROWS:
            for level in SINGLE_LEVELS:
                f = len(srcs)
                s = Src(synth.generate(seed=synth.BASE_SEED + 8900 + f, level=level, rows=rows, nblocks=3, mix=synth.MIX_SINGLE,
                                       single_code=code, pwr_min=12, pwr_max=12))
                srcs.append(s)
                W, bl = s.st.words, s.st.block_len
                # whole, indexed to its end by the host, no index outside its block's range (H1): nothing sends it back to the host reader
                assert (s.ix.blocks, s.ix.end_status, s.marks.size) == (3, 0, 4), (code, rows, level)
                assert (s.st.info.blocks, s.st.info.end_status, s.st.info.npatches) == (3, 0, 0) and W == 3 * bl, (code, rows, level)
                assert (s.st.info.cols, bl) == (1 << level, rows << level), (code, rows, level)
                windows += [(f, 0, W), (f, 2 * bl + bl // 2, W - 2 * bl - bl // 2)]
    return srcs, windows


def test_block_walk_single_fillers(dev):
    """the block-per-wavefront walk (acm_parse.hip: acm_parse_scan_blocks) on streams that hold ONE filler each - the counterpart of
    test_gpu_parity.py::test_device_walk_k_columns, which reaches the stream-per-wavefront kernel only: every k code and every ternary
    code x rows around the 16-row switch of the jump table, one row, tall columns that need several 64-bit windows x columns per block
    below / at / above one wavefront's 64 offsets.  The streams are clean (single_filler_sources), so the device must
    walk every window itself: a fall-back to the host reader would hide a broken walk"""
    srcs, windows = single_filler_sources()
    for parse in BOTH:
        got, st, words, slots, tm = run(dev, srcs, windows, parse)
        assert not any(st) and tm.device_parsed + tm.host_parsed == len(windows)
        assert (tm.host_parsed == 0) == (parse == capi.PARSE_DEVICE) and (tm.device_parsed == 0) == (parse == capi.PARSE_HOST)


def test_truncated_and_foreign_files(dev):
    good = matrix_stream(7, 16, 4)
    srcs = [Src(good), Src(good[:len(good) * 2 // 3]), Src(b"RIFF" + bytes(200)), Src(good[:len(good) // 3]), Src(good[:30]),
            Src(matrix_stream(5, 3, 4))]
    assert srcs[1].st.info.end_status < 0 and srcs[1].st.words > 0 and srcs[2].st is None
    windows = []
    for f, s in enumerate(srcs):
        if s.st is not None and s.st.words > 20:
            windows += [(f, a, n) for a, n in window_kinds(s)]
        else:
            windows += [(f, 0, 100), (f, 5, 0), (f, 1000, 10)]
    for parse in BOTH:
        got, st, words, slots, tm = run(dev, srcs, windows, parse, index=[s.marks for s in srcs])
        by_file = {f: [st[k] for k, w in enumerate(windows) if w[0] == f] for f in range(len(srcs))}
        assert ACM_ERR_NOT_ACM in by_file[2] and srcs[1].st.info.end_status in by_file[1] and set(by_file[0]) == {0}


def test_stale_and_foreign_indices_degrade_to_statuses(dev):
    """an index that does not belong to its file: checked on the host before anything derived from it reaches the device, and by
    the walk against every block - statuses, or still the right PCM; never a fault; the device handle stays usable"""
    a, b = Src(make_stream(6300, 7, 16, 12, mix=1)), Src(make_stream(6301, 7, 16, 12, mix=1))
    bl, W = a.st.block_len, a.st.words
    windows = [(0, 0, 500), (0, 3 * bl + 11, 2 * bl), (0, 7 * bl, bl), (0, W - 300, 300), (1, 2 * bl + 5, 3 * bl), (0, 5 * bl + 1, 40)]
    wrong = []
    m = a.marks.copy()
    m["val"][4] ^= 0x40                                 # a header that is not the block's
    wrong.append(m)
    m = a.marks.copy()
    m["bit"][4] = int(m["bit"][4]) + 3                  # a mark a few bits off
    wrong.append(m)
    m = a.marks.copy()
    m["bit"][8] = int(m["bit"][8]) - 8                  # ... and one a byte early
    wrong.append(m)
    n = min(a.marks.size, b.marks.size)
    if int(b.marks["bit"][n - 1]) <= 8 * len(a.data):
        wrong.append(b.marks[:n].copy())                # the index of another file of the same geometry
    m = a.marks.copy()
    m["bit"][5], m["bit"][6] = a.marks["bit"][6], a.marks["bit"][5]
    wrong.append(m)                                     # not monotone: refused on the host
    for parse in BOTH:
        for m in wrong:
            got, st, words, slots, tm = run(dev, [a, b], windows, parse, index=[m, b.marks], check=False)
            bad = 0
            for k, (f, first, count) in enumerate(windows):
                if st[k] == 0:
                    want = [a, b][f].pcm()[first:first + count]
                    assert words[k] == count and np.array_equal(got[k], want), (k, parse)
                else:
                    assert words[k] == 0, (k, parse)
                    bad += 1
            assert bad >= 1 and st[4] == 0              # the other item's window is unaffected
        run(dev, [a, b], windows, parse)                # the same device, the right index: everything works


def test_auto_chooses_by_staged_blocks(dev):
    """ACM_BATCH_PARSE_AUTO: the host pool for calls that stage fewer than 256 blocks, the device walk from there on (include/acm_hip.h)"""
    srcs = [Src(make_stream(6500 + k, 8, 16, 40, cut=k)) for k in range(4)]
    bl = srcs[0].st.block_len
    small = [(f, 5 * bl + 7, 3 * bl) for f in range(4)]                 # 4 blocks each
    got, st, words, slots, tm = run(dev, srcs, small, capi.PARSE_AUTO)
    assert tm.blocks_parsed < 256 and tm.device_parsed == 0 and tm.host_parsed == 4
    big = [(f, b * bl + 9, 10 * bl) for f in range(4) for b in range(0, 28, 4)]         # 11 blocks each, 28 windows
    got, st, words, slots, tm = run(dev, srcs, big, capi.PARSE_AUTO)
    assert tm.blocks_parsed >= 256 and tm.device_parsed == len(big) and tm.host_parsed == 0


def test_mixed_host_and_device_windows(dev):
    """one call that holds a window the device parser takes and one the host stages from the start: a file chopped by its last byte is
    still whole - its last block ends inside the zero byte the reader appends - but the last mark lies behind the bytes a span can
    have, so the window over the last block stays with the host while the one over the first goes to the device"""
    whole = make_stream(7002, 5, 4, 6)
    s = Src(whole[:-1])
    assert len(s.data) == 459
    assert (s.ix.blocks, s.ix.end_status, s.marks.size) == (6, 0, 7) and int(s.marks["bit"][6]) == 3674 > 8 * len(s.data)
    assert s.st.words == 768 and np.array_equal(s.pcm(), Src(whole).pcm())
    windows = [(0, 0, 200), (0, 5 * 128 + 7, 100)]
    got, st, words, slots, tm = run(dev, [s], windows, capi.PARSE_DEVICE)
    assert tm.device_parsed == 1 and tm.host_parsed == 1
    got, st, words, slots, tm = run(dev, [s], windows, capi.PARSE_HOST)
    assert tm.device_parsed == 0 and tm.host_parsed == 2
    # a window the host stager rejects on that first pass (the header of its last block is not what the index says) has nothing to
    # upload: the call sends the device window's byte span and the two job tables, and that is all
    m = s.marks.copy()
    m["val"][5] ^= 0x40
    got, st, words, slots, tm = run(dev, [s], windows, capi.PARSE_DEVICE, index=[m], check=False)
    assert (st[0], words[0]) == (0, 200) and np.array_equal(got[0], s.pcm()[:200])
    assert st[1] != 0 and words[1] == 0
    assert tm.device_parsed == 1 and tm.host_parsed == 1 and tm.h2d_bytes == h2d_bound([s], windows[:1])


def test_scale_2048_windows(dev):
    """one call, 2048 windows over 512 level-9 streams of 64 blocks mixed with level-7 and level-11 streams"""
    rng = np.random.default_rng(512)
    base = [Src(make_stream(6400 + k, 9, 16, 64, channels=1 + k % 2, cut=k)) for k in range(8)]
    extra = [Src(make_stream(6420 + k, lv, 16, 20, cut=k)) for k, lv in enumerate((7, 11, 7, 11))]
    srcs = [base[k % 8] for k in range(512)] + extra
    windows = []
    for k in range(2048):
        f = int(rng.integers(0, len(srcs)))
        W = srcs[f].st.words
        windows.append((f, int(rng.integers(0, W)), int(rng.integers(1, 22050))))
    for parse in BOTH:
        got, st, words, slots, tm = run(dev, srcs, windows, parse, threads=8)
        assert sum(1 for w in words if w) == 2048
        if parse == capi.PARSE_DEVICE:
            assert tm.device_parsed == 2048 and tm.h2d_bytes <= h2d_bound(srcs, windows)


@pytest.mark.parametrize("f32", [False, True])
def test_gpu_decoder_crop(f32):
    import torch
    from libacm_amd import batch
    files = [matrix_stream(lv, rows, 5) for lv, rows in ((5, 16), (8, 16), (9, 3), (11, 4))] + [b"no acm"]
    dec = batch.GpuDecoder(0, parse=capi.PARSE_DEVICE, dtype=torch.float32 if f32 else torch.int16)
    index = batch.build_index(files, threads=2)
    whole, offs, words, sts = dec(files)
    whole = whole.cpu().numpy()
    windows = [(0, 0, 100), (1, 1000, 5000), (2, 77, 3000), (3, 4099, 9000), (1, words[1] - 10, 50), (4, 0, 10), (2, 5, 0), (0, 33, 64)]
    for parse in (capi.PARSE_HOST, capi.PARSE_DEVICE, capi.PARSE_AUTO):
        dec.parse = parse
        pcm, o, n, st = dec.crop(files, windows, index)
        pcm = pcm.cpu().numpy()
        assert pcm.dtype == (np.float32 if f32 else np.int16)
        for k, (f, first, count) in enumerate(windows):
            want = whole[offs[f] + first:offs[f] + min(first + count, words[f])] if first < words[f] else whole[:0]
            assert n[k] == want.size and np.array_equal(pcm[o[k]:o[k] + n[k]].view(np.uint8), want.view(np.uint8)), k
            assert st[k] == (0 if n[k] == count else sts[f])
    dec.dev.close()
