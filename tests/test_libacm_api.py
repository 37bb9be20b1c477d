"""The drop-in libacm.h API of libacm_hip.so against the golden traces of the reference.

CPU part: everything that only needs the host parser (open/close ownership, header errors, getters,
seeking with decode-and-discard, truncation bookkeeping).  GPU part (-m gpu): the PCM itself."""
import ctypes as C

import pytest

import oracle_api as O
from helpers import RefAnswers, decode_record, golden, golden_file, sha
from libacm_amd import capi


def ours(data, force_chans=0, **io_kw):
    return O.LibacmStream(O.bind_libacm(capi.lib()), data, force_chans, **io_kw)


# ------------------------------------------------------------------ CPU
def test_open_errors_and_ownership():
    for case in golden()["F6_headers"] + golden()["F5_wavc"]["bad"]:
        s = ours(golden_file(case["file"]))
        assert s.err == (case["open"] if case["open"] < 0 else 0), case["file"]
        if s.err < 0:
            assert s.io.closed == 0         # on failure the caller keeps its handle (decode.c:817-823)
        else:
            s.close()
            assert s.io.closed == 1         # on success acm_close runs close_func once (decode.c:882-883)
    capi.lib().acm_close(None)              # acm_close(NULL) is a no-op


def test_read_func_contract():
    s = ours(golden_file("f7_src"))
    assert s.io.read_calls and all(c == (1, 65536) for c in s.io.read_calls)   # decode.c:51
    s.close()


def test_getters_after_open():
    g = golden()["F7_api"]["getters"]
    src = golden_file("f7_src")
    for label, fc, kw in (("plain", 0, {}), ("force1", 1, {}), ("force2", 2, {}), ("nolen", 0, {"with_length": False})):
        s = ours(src, fc, **kw)
        for k, v in g[label].items():
            got = s.info() if k == "info" else s.getter(k)
            assert got == v, (label, k, got, v)
        s.close()


def test_seek_and_discard_bookkeeping():
    """acm_seek_pcm / acm_seek_time / acm_read(NULL) positions, incl. acm_raw_tell (util.c:192-253)"""
    g = golden()["F7_api"]
    s = ours(golden_file("f7_src"))
    for step in g["seeks"]:
        if step["op"] == "read":
            rc, _ = s.read(step["arg"], discard=True)
            assert (rc, s.getter("pcm_tell")) == (step["rc"], step["pcm_tell"]), step
        else:
            rc = s.seek_pcm(step["arg"]) if step["op"] == "pcm" else s.seek_time(step["arg"])
            assert (rc, s.getter("pcm_tell"), s.getter("raw_tell")) == (step["rc"], step["pcm_tell"], step["raw_tell"]), step
    s.close()
    s = ours(golden_file("f7_src"), seekable=False)
    s.read(256, discard=True)
    assert s.seek_pcm(0) == g["noseek_back"] == -8
    assert s.seek_pcm(300) == g["noseek_fwd"]
    s.close()
    s = ours(golden_file("f7_src"))
    assert [s.read(64, wordlen=1, discard=True)[0], s.read(64, wordlen=4, discard=True)[0]] == g["bad_wordlen"]
    s.close()


@pytest.mark.parametrize("shape", [(5, 4, 60, 1, 0), (7, 16, 25, 2, 0), (3, 1, 90, 1, 0), (6, 5, 40, 2, 1), (0, 3, 50, 1, 0), (7, 16, 500, 1, 1)])
def test_random_seek_walk_matches_reference(shape, monkeypatch):
    """a walk of forward/backward acm_seek_pcm / acm_seek_time calls and discard reads: return values, acm_pcm_tell,
    acm_raw_tell and acm_time_tell equal the reference's at every step - with the block index (backward seeks re-enter
    the stream near the target) and without it (acmhip_set_seek_index(0): rewind and re-parse, as the reference does).  The
    reference's side is replayed from tests/golden/ref_answers.json (helpers.RefAnswers)"""
    import numpy as np
    from libacm_amd import synth
    level, rows, nb, ch, wavc = shape
    f = synth.generate(seed=synth.BASE_SEED + 4200 + level, level=level, rows=rows, nblocks=nb, channels=ch, wavc=wavc,
                       total_values=nb * (rows << level) - 3 * ch)
    total_pcm = (nb * (rows << level) - 3 * ch) // ch
    reads_with_index = None
    for no_index in (False, True):
        if no_index:
            seek_index(False, monkeypatch)
        rng = np.random.default_rng(level * 100 + rows)
        ans = RefAnswers("test_libacm_api::test_random_seek_walk_matches_reference[%s]%s" % (shape, " no_index" if no_index else ""))
        r = O.LibacmStream(O.ref_lib(), f) if ans.live else None
        s = ours(f)
        for step in range(60):
            op = int(rng.integers(0, 3))
            if op == 0:
                n = int(rng.integers(1, 4000)) * 2
                got, want = s.read(n, discard=True)[0], ans.ask(lambda: r.read(n, discard=True)[0])
            elif op == 1:
                pos = int(rng.integers(0, total_pcm + 50))
                got, want = s.seek_pcm(pos), ans.ask(lambda: r.seek_pcm(pos))
            else:
                ms = int(rng.integers(0, total_pcm * 1000 // 22050 + 20))
                got, want = s.seek_time(ms), ans.ask(lambda: r.seek_time(ms))
            state = [s.getter("pcm_tell"), s.getter("raw_tell"), s.getter("time_tell")]
            want_state = ans.ask(lambda: [r.getter("pcm_tell"), r.getter("raw_tell"), r.getter("time_tell")])
            assert got == want and state == want_state, (shape, no_index, step, op, got, want, state, want_state)
        if no_index:
            # the index must have saved re-parsing: fewer refill calls than the rewind-and-re-parse flavour (long files)
            if len(f) > 200000:
                assert reads_with_index < len(s.io.read_calls)
        else:
            reads_with_index = len(s.io.read_calls)
        s.close()
        if r is not None:
            r.close()
        ans.done()


def discard_all(s):
    words = 0
    while True:
        rc, _ = s.read(8192, discard=True, loop=True)
        if rc <= 0:
            return words, rc
        words += rc // 2


def test_truncation_every_byte_discard():
    g = golden()["F4_truncation"]
    base = golden_file(g["file"])
    for cut in g["cuts"]:
        s = ours(base[:cut["len"]])
        assert s.err == (cut["open"] if cut["open"] < 0 else 0)
        if s.err == 0:
            words, rc = discard_all(s)
            assert (words, rc, s.getter("raw_tell")) == (cut["words"], cut["status"], cut["raw_tell_end"]), cut
            s.close()


def test_short_reads_and_read_errors_discard():
    g = golden()["F7_api"]
    src = golden_file("f7_src")
    for sr in g["short_reads"]:
        s = ours(src, max_read=sr["max_read"])
        assert s.err == (sr["open"] if sr["open"] < 0 else 0), sr
        if s.err == 0:
            words, rc = discard_all(s)
            assert (words, rc) == (sr["words"], sr["status"]), sr
            s.close()
    for re_ in g["read_errors"]:
        s = ours(src, fail_read_at=re_["fail_at"])
        assert s.err == (re_["open"] if re_["open"] < 0 else 0), re_
        if s.err == 0:
            words, rc = discard_all(s)
            assert (words, rc) == (re_["words"], re_["status"]), re_
            s.close()


def test_window_buffers_follow_the_file_not_its_header():
    """a header may promise 2^32 - 1 samples (decode.c:734-738 takes it as it is); the read-ahead buffers of the stream are sized by
    what the data source can hold when it says how long it is, and by a 4-Msample window when it does not (they were
    256 MB per open stream for such a file).  Decode-and-discard never touches a device, so this runs anywhere."""
    import os
    from helpers import make_stream

    def vm_kb():
        return int(open("/proc/self/statm").read().split()[0]) * os.sysconf("SC_PAGE_SIZE") // 1024
    good = make_stream(4400, 9, 16, 6)
    lying = bytearray(good)
    lying[4:8] = (0xFFFFFFFF).to_bytes(4, "little")
    for kw, limit_kb in (({}, 8 << 10), ({"with_length": False}, 40 << 10)):
        before = vm_kb()
        streams = [ours(bytes(lying), **kw) for _ in range(4)]
        for s in streams:
            assert s.err == 0
            rc, _ = s.read(4096, discard=True)          # parses the first window (acm_read(NULL): decode.c:859-866)
            assert rc == 4096
        grown = (vm_kb() - before) // 4
        for s in streams:
            words = 2048
            while True:                                 # ... and the stream still ends where its bytes end
                rc, _ = s.read(1 << 20, discard=True)
                if rc <= 0:
                    break
                words += rc // 2
            assert words == 6 * 16 * 512
            s.close()
        assert grown < limit_kb, (kw, grown)


def test_corrupt_streams_discard():
    for case in golden()["F3_corrupt"]:
        s = ours(golden_file(case["file"]))
        assert s.err == 0
        words, rc = discard_all(s)
        assert (words, rc) == (case["words"], case["status"]), case["file"]
        s.close()
    gl = golden()["F7_api"]["loop_swallow"]
    s = ours(golden_file(gl["file"]))
    assert [s.read(4096, discard=True, loop=True)[0] for _ in range(3)] == gl["rc"]
    s.close()


def seek_index(on, monkeypatch):
    """acmhip_set_seek_index (include/acm_hip.h) for the rest of the test: monkeypatch undoes it through the property's setter"""
    monkeypatch.setattr(_SEEK, "on", on)


class _SeekState:
    def __init__(self):
        object.__setattr__(self, "_on", True)

    @property
    def on(self):
        return self._on

    @on.setter
    def on(self, v):
        object.__setattr__(self, "_on", v)
        capi.lib().acmhip_set_seek_index(1 if v else 0)        # monkeypatch's undo sets it back through here


_SEEK = _SeekState()


# ------------------------------------------------------------------ PCM: on the device (-m gpu) and on the host
@pytest.fixture(params=["host", pytest.param("device", marks=pytest.mark.gpu)])
def side(request):
    """Where acm_read() synthesises: "device" - the GPU, whatever the stream's length (acmhip_set_host_synth_limit(0); -m gpu) -
    or "host" - the library's own host synthesis (libacm_amd/csrc/acm_host_synth.cpp; what a box without a GPU gets, and short streams
    by default).  Same goldens, same oracle, bit for bit."""
    L = capi.lib()
    L.acmhip_set_host_synth_limit.argtypes = [C.c_uint64]
    L.acmhip_set_host_synth_limit.restype = None
    L.acmhip_host_synth_limit.restype = C.c_uint64
    prev = L.acmhip_host_synth_limit()
    if request.param == "device":
        request.getfixturevalue("dev")
        L.acmhip_set_host_synth_limit(0)
    else:
        L.acmhip_set_host_synth_limit(2 ** 64 - 1)
    yield request.param
    L.acmhip_set_host_synth_limit(prev)


@pytest.mark.parametrize("family", ["F1_matrix", "F2_codes", "F3_corrupt", "F6_headers"])
def test_pcm_families(side, family):
    for case in golden()[family]:
        rec = decode_record(ours, golden_file(case["file"]))
        for k in ("open", "status", "words", "sha256", "info", "raw_tell_end"):
            if k in case:
                assert rec.get(k) == case[k], (case["file"], k)


def test_pcm_truncation_every_byte(side):
    g = golden()["F4_truncation"]
    base = golden_file(g["file"])
    for cut in g["cuts"]:
        rec = decode_record(ours, base[:cut["len"]])
        for k in ("open", "status", "words", "sha256", "raw_tell_end"):
            assert rec.get(k) == cut[k], (cut["len"], k)


def test_pcm_wavc_and_quirk(side):
    g = golden()["F5_wavc"]
    for k, fc in (("plain", 0), ("wavc", 0), ("wavc_quirk", -1), ("plain_quirk", -1)):
        rec = decode_record(ours, golden_file(g[k]["file"]), fc)
        assert (rec["sha256"], rec["words"], rec["info"]) == (g[k]["sha256"], g[k]["words"], g[k]["info"])


def test_pcm_api_traces(side):
    g = golden()["F7_api"]
    src = golden_file("f7_src")
    s = ours(src)
    for step in g["reads"]:
        rc, b = s.read(step["ask"])
        assert (rc, sha(b), s.getter("pcm_tell"), s.getter("raw_tell"), s.getter("time_tell")) == \
               (step["rc"], step["sha"], step["pcm_tell"], step["raw_tell"], step["time_tell"]), step
    s.close()
    for f in g["formats"]:
        rec = decode_record(ours, src, be=f["be"], sgned=f["sgned"])
        assert (rec["sha256"], rec["words"]) == (f["sha256"], f["words"])
    s = ours(src)
    for step in g["seeks"]:
        if step["op"] == "read":
            rc, b = s.read(step["arg"])
            assert (rc, sha(b), s.getter("pcm_tell")) == (step["rc"], step["sha"], step["pcm_tell"]), step
        else:
            rc = s.seek_pcm(step["arg"]) if step["op"] == "pcm" else s.seek_time(step["arg"])
            assert (rc, s.getter("pcm_tell"), s.getter("raw_tell")) == (step["rc"], step["pcm_tell"], step["raw_tell"]), step
    s.close()
    gl = g["loop_swallow"]
    s = ours(golden_file(gl["file"]))
    rc1, b1 = s.read(4096, loop=True)
    assert [rc1, s.read(4096, loop=True)[0], s.read(4096, loop=True)[0]] == gl["rc"] and sha(b1) == gl["sha"]
    s.close()


def test_format_switch_mid_stream(side):
    """the window is re-synthesised when a caller changes the sample layout between reads"""
    src = golden_file("f7_src")
    want = {}
    for be in (0, 1):
        for sg in (0, 1):
            o = O.Oracle(src)
            want[(be, sg)] = o.read(1 << 20, be=be, sgned=sg, loop=True)[1]
            o.close()
    s = ours(src)
    pos = 0
    for k, (be, sg) in enumerate([(0, 1), (1, 1), (0, 0), (1, 0), (0, 1), (1, 0)] * 4):
        rc, b = s.read(40 + 2 * k, be=be, sgned=sg)
        assert rc > 0 and b == want[(be, sg)][pos:pos + rc]
        pos += rc
    s.close()


def test_long_stream_many_windows(side):
    """windows grow 64K -> 4M samples; the carry (2 staged rows) must make window seams invisible"""
    from helpers import make_stream, oracle_pcm
    for lv, rows, nb in ((7, 16, 4000), (9, 16, 700), (3, 1, 30000), (11, 5, 60), (0, 1, 5000)):
        f = make_stream(2000 + lv, lv, rows, nb, cut=11)
        rec = decode_record(ours, f)
        want, st = oracle_pcm(f)
        assert rec["words"] == want.size and rec["sha256"] == sha(want.tobytes()) and rec["status"] == st


def test_concurrent_streams_share_the_device(side):
    """several threads, each decoding its own stream through acm_read on the shared default device
    (reference contract: one ACMStream = one thread at a time, distinct streams independent)"""
    import threading
    from helpers import make_stream, oracle_pcm
    files = [make_stream(2600 + k, [7, 9, 5, 11][k % 4], [16, 16, 3, 4][k % 4], [300, 60, 900, 12][k % 4], channels=1 + k % 2)
             for k in range(8)]
    want = [oracle_pcm(f)[0].tobytes() for f in files]
    got = [None] * len(files)

    def work(k):
        s = ours(files[k])
        out = []
        ask = [8192, 4000, 123456, 4][k % 4]      # (a 2-byte request on a stereo stream yields 0, as in the reference)
        while True:
            rc, b = s.read(ask, loop=True)
            if rc <= 0:
                break
            out.append(b)
        s.close()
        got[k] = b"".join(out)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(len(files))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert got == want


def test_interleaved_reads_on_two_streams(side):
    """alternate small reads on two open streams: windows, carries and plans must not leak between them"""
    from helpers import make_stream, oracle_pcm
    fa, fb = make_stream(2700, 7, 16, 200), make_stream(2701, 9, 3, 150, channels=2)
    wa, wb = oracle_pcm(fa)[0].tobytes(), oracle_pcm(fb)[0].tobytes()
    a, b = ours(fa), ours(fb)
    ga, gb = [], []
    for k in range(100000):
        ra, xa = a.read(3000 + (k % 7) * 2)
        rb, xb = b.read(5000 - (k % 5) * 4)
        ga.append(xa)
        gb.append(xb)
        if ra <= 0 and rb <= 0:
            break
    a.close()
    b.close()
    assert b"".join(ga) == wa and b"".join(gb) == wb


def test_acm_read_writes_no_byte_beyond_the_request(side):
    """acm_read(buf, n) into a buffer of n bytes + 64 guard bytes: requests of a sample, three samples, just below and above a 4 KB
    page and far beyond one read-ahead window's first rows, on a mono and a stereo stream, with a seek between the reads - the guard
    bytes stay as they were, return values and bytes are the oracle's"""
    from helpers import make_stream
    L = O.bind_libacm(capi.lib())
    for ch, (lv, rows, nb) in ((1, (7, 16, 90)), (2, (9, 5, 44))):
        f = make_stream(2800 + ch, lv, rows, nb, channels=ch, cut=3 * ch)
        s, o = ours(f), O.Oracle(f)
        assert s.err == 0 and o.err == 0
        for k, n in enumerate((2, 6, 4094, 4098, 123458, 4098, 6, 4094)):
            if k == 5:
                pos = 1237 if ch == 1 else 30011
                assert s.seek_pcm(pos) == o.seek_pcm(pos) == pos
            be, sg = k % 2, 1 - (k // 2) % 2
            buf = (C.c_uint8 * (n + 64))()
            C.memset(buf, 0xA5, n + 64)
            rc = L.acm_read(s.h, buf, n, be, 2, sg)
            want_rc, want = o.read(n, be=be, sgned=sg)
            assert rc == want_rc and (rc > 0 or (ch == 2 and n == 2)), (ch, k, n, rc, want_rc)
            assert bytes(buf[:max(rc, 0)]) == want, (ch, k, n)
            assert bytes(buf[n:]) == b"\xA5" * 64, (ch, k, n)
            assert s.getter("pcm_tell") == o.getter("pcm_tell")
        s.close()
        o.close()


def read_digest(rc_bytes):
    """(rc, PCM bytes) of one read -> [rc, sha256 of the bytes], the form the reference's recorded answers take"""
    return [rc_bytes[0], sha(rc_bytes[1])]


@pytest.mark.parametrize("shape", [(7, 16, 120, 1, 0), (5, 1, 300, 2, 1), (9, 16, 12, 2, 0), (6, 3, 80, 1, 0),
                                   (11, 3, 40, 1, 0), (12, 5, 10, 2, 0), (13, 2, 12, 2, 0), (14, 1, 8, 1, 1), (15, 2, 5, 2, 1)])
def test_random_seek_walk_pcm(side, shape):
    """seeks forward and backward (block index in use) followed by real reads: the PCM bytes and all positions equal
    the reference's (replayed from tests/golden/ref_answers.json).  On the device side the shapes of levels 11-15 are the seeks into the
    stage-wise and the prefix + plane kernels that are held to the reference itself"""
    import numpy as np
    from libacm_amd import synth
    level, rows, nb, ch, wavc = shape
    total = nb * (rows << level) - 5 * ch
    f = synth.generate(seed=synth.BASE_SEED + 4300 + level, level=level, rows=rows, nblocks=nb, channels=ch, wavc=wavc,
                       total_values=total)
    rng = np.random.default_rng(level * 7 + rows)
    ans = RefAnswers("test_libacm_api::test_random_seek_walk_pcm[%s]" % (shape,))
    r = O.LibacmStream(O.ref_lib(), f) if ans.live else None
    s = ours(f)
    for step in range(50):
        if step % 2 == 0:
            pos = int(rng.integers(0, total // ch))
            assert s.seek_pcm(pos) == ans.ask(lambda: r.seek_pcm(pos)), (shape, step, pos)
        n = int(rng.integers(1, 3000)) * 2 * ch
        be, sg = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        got, want = read_digest(s.read(n, be=be, sgned=sg)), ans.ask(lambda: read_digest(r.read(n, be=be, sgned=sg)))
        assert got == want, (shape, step, n)
        assert [s.getter(k) for k in ("pcm_tell", "raw_tell")] == ans.ask(lambda: [r.getter(k) for k in ("pcm_tell", "raw_tell")])
    s.close()
    if r is not None:
        r.close()
    ans.done()


@pytest.mark.parametrize("no_index", [False, True])
def test_seek_walk_on_a_stale_table_stream(side, no_index, monkeypatch):
    """hazard H1 plus seeks: out-of-range indices read table entries left by earlier blocks, the reference never clears its
    table (decode.c:809-810) and has only decoded what it served - our parser reads ahead of the caller, so a backward
    seek must continue from the table as the SERVED blocks left it.  prime_table makes block 0 write every
    entry, so the reference's answer does not depend on heap garbage.  Its answers are replayed from tests/golden/ref_answers.json."""
    import numpy as np
    from libacm_amd import synth
    if no_index:
        seek_index(False, monkeypatch)
    level, rows, nb = 6, 5, 200
    total = nb * (rows << level) - 3
    f = synth.generate(seed=synth.BASE_SEED + 4400, level=level, rows=rows, nblocks=nb, total_values=total, mix=1,
                       allow_out_of_range=1, prime_table=1, pwr_min=0, pwr_max=7)
    rng = np.random.default_rng(99)
    ans = RefAnswers("test_libacm_api::test_seek_walk_on_a_stale_table_stream[%s]" % ("no_index" if no_index else "index"))
    r = O.LibacmStream(O.ref_lib(), f) if ans.live else None
    s = ours(f)
    pos_list = [total // 2, 100, total // 3, 5000, total - 4000, 0, total // 4]
    for step, pos in enumerate(pos_list):
        # a short read first: our read-ahead window is far ahead of what has been served when the seek comes
        n = int(rng.integers(1, 400)) * 2
        assert read_digest(s.read(n)) == ans.ask(lambda: read_digest(r.read(n))), ("pre", step)
        assert s.seek_pcm(pos) == ans.ask(lambda: r.seek_pcm(pos)), (step, pos)
        n = int(rng.integers(2000, 9000)) * 2
        assert read_digest(s.read(n)) == ans.ask(lambda: read_digest(r.read(n))), (step, pos, n)
    s.close()
    if r is not None:
        r.close()
    ans.done()
