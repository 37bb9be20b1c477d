"""Leftovers in reused device memory must not pass a GPU test.

A device handle's staging arenas are grow-only and reused by every batch, window and index call (acmhip_arena_get), and the device blocks
of destroyed plans go to the next plan: a call works at the addresses - and, the layout being a function of the headers, at the offsets - of
the call before it.  A kernel that skips a column, a pair-table entry nobody wrote or a read-back that was dropped then finds the previous
call's bytes, which for a suite that decodes the same files twice are the right ones.  The handle's fill mode (include/acm_hip.h:
acmhip_device_set_fill) takes that away, and tests/helpers.py turns it on for every GPU test through capi.FILL_MODE.  Here:

  * the control: with the mode off the arena of the next call holds the previous call's indices, element for element;
  * the mode itself: every arena a decode used comes back from the library's own acmhip_arena_lock / acmhip_arena_get filled over exactly
    the bytes asked for - 0xA5 bytes in the PCM arenas, 0x5A bytes in the int16 index arenas, zeros everywhere else - and a plan built
    from recycled blocks decodes exactly;
  * the device parser's arena contract, checkable now that the arena in front of the call is known: the int16 and header arenas hold
    what the host stager stages, element for element, and nothing outside the streams' slices is touched; the byte-plane arena and its
    pair table give the staged indices back through acmhip_mform_unrows, the int16 arena holds only the rows from mf_rows - 2 on, and
    what belongs to no stream keeps the fill;
  * the orders the suite never ran: device parsing before host parsing, 3 block ranges before 1, byte planes before int16 staging,
    float32 before int16 output, on one fresh handle, each against the oracle;
  * capi.synth poisons its PCM buffer: a stream left out of a plan's descriptors comes back as poison, not as the PCM of the call before.

One population throughout, about 40 small streams: the smallest shapes that still reach the walk and the column kernel, every width
class of the byte-plane form the device parser writes (8 bits, two bytes, the whole range), row pairs across blocks of odd height, parked
pair-table entries (a truncated stream), and the chunk, lean-tile, fused, register and prefix synthesis kernels."""
import ctypes as C

import numpy as np
import pytest

import test_batch_layout as BL
from helpers import make_stream, oracle_pcm
from libacm_amd import capi

pytestmark = pytest.mark.gpu

LEVELS, HEIGHTS = (3, 5, 8, 9, 12, 13), (1, 3, 16)
IDX_FILL = np.int16(0x5A5A)
HALF_BYTES = {0: 4, 1: 3, 2: 2, 3: 4}           # bytes per index, times two, by class code of the six-stage byte-plane form


class Pop:
    """the population: files, what the host stager makes of each (None: not ACM), the oracle's PCM and status"""

    def __init__(self):
        files = []
        for k, (level, rows) in enumerate((lv, r) for lv in LEVELS for r in HEIGHTS):
            for ch in (1, 2):
                # 2 - 8 blocks; the chunk kernel's levels get enough rows for a few whole tiles whatever the block height
                nb = 2 + (3 * k + ch) % 7 if rows > 1 or level < 8 else 8
                files.append(make_stream(52000 + 2 * k + ch, level, rows, nb, channels=ch, cut=1 + (k + ch) % 7, pwr_max=12))
        self.truncated = len(files)
        files.append(files[2 * (3 * 3 + 2)][:len(files[2 * (3 * 3 + 2)]) * 2 // 3])                # level 9, 16 rows: ends inside a block
        self.not_acm = len(files)
        files.append(b"not an acm file")
        self.h1 = len(files)
        files.append(make_stream(52100, 9, 16, 4, mix=1, allow_out_of_range=1, prime_table=1, pwr_min=0, pwr_max=6))
        self.loud = len(files)
        files.append(make_stream(52101, 9, 16, 4, mix=2, single_code=16, pwr_min=15, pwr_max=15, val_min=65535, val_max=65535))
        self.files = files
        self.staged = [capi.stage_file(f) if k != self.not_acm else None for k, f in enumerate(files)]
        self.want = [oracle_pcm(f) if k != self.not_acm else (np.zeros(0, np.uint16), None) for k, f in enumerate(files)]
        assert self.staged[self.h1].patches is not None and len(self.staged[self.h1].patches) > 0
        assert 0 < self.want[self.truncated][0].size < self.want[2 * (3 * 3 + 2)][0].size and self.want[self.truncated][1] != 0
        assert int(self.staged[self.loud].hdr[:, 0].max()) == 65535 and int(self.staged[self.loud].hdr[:, 1].min()) == 15

    def clean(self, k):
        """does the device walk keep stream k (every block the header promises is there, no H1 patch)?"""
        return k not in (self.truncated, self.not_acm, self.h1)


@pytest.fixture(scope="module")
def pop():
    return Pop()


def check_batch(pop, res, what):
    """(status, PCM) per file of a host-output batch call against the oracle"""
    for k, (status, pcm) in enumerate(res):
        want, wst = pop.want[k]
        if k == pop.not_acm:
            assert status != 0 and pcm.size == 0, what
            continue
        assert status == wst and pcm.size == want.size and np.array_equal(pcm, want), (what, k, status, wst, pcm.size, want.size)
    assert res[pop.truncated][0] != 0


def layout(pop, flags, plan_flags, parse, threads=4):
    """the layout acm_batch_decode computes for the population with host output (acmk_batch_layout_visit), decoded as
    tests/test_batch_layout.py decodes it"""
    L = BL._lib()
    n = len(pop.files)
    info = (capi.StageInfo * n)()
    length, ok, has_pcm = (C.c_uint64 * n)(), (C.c_uint8 * n)(), (C.c_uint8 * n)()
    for k, f in enumerate(pop.files):
        rc, info[k] = capi.probe(f)
        length[k], ok[k], has_pcm[k] = len(f), rc == 0, rc == 0 and info[k].total_values > 0
    opts = capi.BatchOpts(0, 0, threads, plan_flags, parse, flags, None, 0, None)
    tables, elem = {}, {}

    def visit(_ctx, name, data, elem_bytes, count):
        tables[name.decode()] = C.string_at(data, elem_bytes * count)
        elem[name.decode()] = elem_bytes
    rc = L.acmk_batch_layout_visit(info, length, ok, has_pcm, n, C.byref(opts), threads, 0, BL.VISIT(visit), None)
    assert rc == 0
    return BL.decode({"rc": rc, "tables": tables, "elem": elem})


def arena_api():
    L = capi.lib()
    L.acmhip_arena_lock.argtypes = L.acmhip_arena_unlock.argtypes = [C.c_void_p]
    L.acmhip_arena_lock.restype = L.acmhip_arena_unlock.restype = None
    L.acmhip_arena_get.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
    return L


def read_slot(dev, ptr, nbytes, is_host):
    """`nbytes` bytes of a staging arena: pinned host memory as it is, device memory downloaded"""
    if is_host:
        return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=np.uint8).copy()
    out = np.zeros(nbytes, np.uint8)
    dev.download(out, ptr)
    return out


def read_arena(dev, name, dtype):
    slot, ptr, nbytes, is_host, fill = dev.arena_info()[name]
    assert ptr and nbytes, name
    return read_slot(dev, ptr, nbytes, is_host)[:nbytes // np.dtype(dtype).itemsize * np.dtype(dtype).itemsize].view(dtype)


def check_int16_arenas(pop, lay, d_idx, d_hdr, dirty_too, first_row=None):
    """every stream's slice of the int16 index arena and of the header arena is what capi.stage_file stages, element for element, over
    the blocks that were staged; -> the mask of the index arena's elements that lie in some stream's reservation.  first_row[k]: the
    first row of stream k the arena has to hold (byte-plane staging: the rows in front of it stay unwritten)"""
    inside = np.zeros(d_idx.size, bool)
    hdr_inside = np.zeros(d_hdr.shape[0], bool)
    for k, s in enumerate(pop.staged):
        slot = lay["slots"][k]
        if not slot["ok"]:
            assert k == pop.not_acm
            continue
        bl, cols = s.block_len, s.info.cols
        io, ho, need = int(slot["idx_off"]), int(slot["hdr_off"]), int(slot["need_blocks"])
        inside[io:io + need * bl] = True
        hdr_inside[ho:ho + need] = True
        assert io + int(slot["idx_len"]) <= d_idx.size and s.info.blocks <= need
        if not pop.clean(k) and not dirty_too:
            continue
        if pop.clean(k):
            assert s.info.blocks == need, k
        lo = (first_row[k] if first_row else 0) * cols
        n = s.info.blocks * bl
        bad = np.nonzero(d_idx[io + lo:io + n] != s.idx[lo:n])[0]
        assert bad.size == 0, "stream %d (level %d, %d rows, %d blocks): %d staged indices differ, first at sample %d (row %d)" % (
            k, s.info.level, s.info.rows, s.info.blocks, bad.size, lo + bad[0], (lo + bad[0]) // cols)
        assert np.array_equal(d_hdr[ho:ho + s.info.blocks], s.hdr[:s.info.blocks]), ("block headers", k)
        if lo:
            assert (d_idx[io:io + lo] == IDX_FILL).all(), ("int16 rows in front of the byte-plane rows were written", k)
    assert hdr_inside[:lay["totals"]["hdr_total"]].all()
    return inside


# ---------------------------------------------------------------------------------------------------------------- the hazard (control)

def test_without_the_mode_the_next_call_starts_on_the_previous_indices(pop, monkeypatch):
    """What the suite stood on: mode OFF, a handle of its own.  After a decode the D_IDX arena holds the population's staged indices, and
    the next holder of the arenas (acmhip_arena_lock / acmhip_arena_get, as the next call takes them) is handed exactly those bytes"""
    monkeypatch.setattr(capi, "FILL_MODE", False)
    L = arena_api()
    flags = capi.BATCH_STAGE_INT16 | capi.batch_ranges(1)
    lay = layout(pop, flags, 0, capi.PARSE_DEVICE)
    with capi.Device(0) as d:
        res, tm = capi.batch_decode(d, pop.files, parse=capi.PARSE_DEVICE, threads=4, byteplane=False, batch_flags=capi.batch_ranges(1))
        check_batch(pop, res, "control")
        assert not getattr(d, "fill", False) and tm.device_parsed >= len(pop.files) - 4
        slot, ptr, nbytes, is_host, fill = d.arena_info()["D_IDX"]
        assert nbytes == 2 * lay["totals"]["idx_total"] and not is_host
        before = read_arena(d, "D_IDX", np.int16)
        L.acmhip_arena_lock(d.h)
        try:
            p = C.c_void_p()
            assert L.acmhip_arena_get(d.h, slot, nbytes, C.byref(p)) == 0 and p.value == ptr
            after = read_slot(d, ptr, nbytes, False).view(np.int16)
        finally:
            L.acmhip_arena_unlock(d.h)
    assert np.array_equal(before, after)
    for k, s in enumerate(pop.staged):
        if pop.clean(k):
            io = int(lay["slots"][k]["idx_off"])
            assert np.array_equal(after[io:io + s.idx.size], s.idx), k            # not zeros, not a pattern: the previous call's right answer
    assert sum(int(np.count_nonzero(s.idx)) for k, s in enumerate(pop.staged) if pop.clean(k)) > 100000


# ---------------------------------------------------------------------------------------------------------------- the mode itself

def test_with_the_mode_every_arena_starts_a_call_filled(pop):
    """mode ON (the switch of tests/helpers.py turns it on for the handle): after the same decode - and one with host parsing, ranges and
    the index, so that every slot has been used - the next holder gets every slot the calls used filled over the bytes they asked for"""
    assert capi.FILL_MODE
    L = arena_api()
    with capi.Device(0) as d:
        seen = {}
        for kw in (dict(parse=capi.PARSE_DEVICE, byteplane=False, batch_flags=capi.batch_ranges(1)),
                   dict(parse=capi.PARSE_DEVICE, flags=capi.PLAN_LEAN_ALWAYS, batch_flags=capi.batch_ranges(3), index=True),
                   dict(parse=capi.PARSE_HOST, flags=capi.PLAN_LEAN_ALWAYS), dict(parse=capi.PARSE_HOST, packed=True, flags=capi.PLAN_LEAN_ALWAYS)):
            check_batch(pop, capi.batch_decode(d, pop.files, threads=4, **kw)[0], kw)
            assert d.fill
            for name, (slot, ptr, nbytes, is_host, fill) in d.arena_info().items():
                if nbytes:
                    seen[name] = (slot, max(nbytes, seen.get(name, (0, 0))[1]), is_host, fill)
        print(sorted(seen))
        assert len(seen) >= 16, sorted(seen)          # nearly every slot has been through a call
        pcm = read_arena(d, "D_PCM", np.uint16)
        assert (pcm != capi.POISON16).sum() > pcm.size // 2             # (the arenas do hold a call's data until the next one takes them)
        info = d.arena_info()
        L.acmhip_arena_lock(d.h)
        try:
            for name, (slot, nbytes, is_host, fill) in sorted(seen.items()):
                nbytes = min(nbytes, 1 << 28)
                p = C.c_void_p()
                assert L.acmhip_arena_get(d.h, slot, nbytes, C.byref(p)) == 0 and p.value == info[name][1], name
                assert fill == (0xA5 if name in ("D_PCM", "H_PCM") else 0x5A if name in ("D_IDX", "H_IDX") else 0), name
                got = read_slot(d, p.value, nbytes, is_host)
                assert (got == fill).all(), "%s: %d of %d bytes are not the fill 0x%02X" % (name, int((got != fill).sum()), nbytes, fill)
                # a second request inside the same hold must not wipe what the holder has written since
                if is_host:
                    C.memset(p.value, 0x11, 16)
                else:
                    d.memset(p.value, 0x11, 16)
                    d.sync()
                assert L.acmhip_arena_get(d.h, slot, nbytes, C.byref(p)) == 0
                assert (read_slot(d, p.value, 16, is_host) == 0x11).all(), name
        finally:
            L.acmhip_arena_unlock(d.h)
        assert d.set_fill(False) is True and d.set_fill(True) is False


def test_a_plan_of_recycled_blocks_decodes_exactly(pop):
    """plans come and go on one handle: the stage-wise planes, the tile tables and the lead-in sink of a plan are the blocks of the plans
    destroyed before it.  Every launch - stage-wise, lean with a sink, stage-wise again over other streams - goes into a poisoned PCM
    buffer (capi.synth does that with the switch on) and is the oracle's PCM"""
    keep = [k for k in range(len(pop.files)) if k != pop.not_acm]
    with capi.Device(0) as d:
        for flags, ks in ((capi.PLAN_STAGEWISE, keep), (capi.PLAN_LEAN_ALWAYS, keep[6:]), (capi.PLAN_STAGEWISE, keep[::-1]),
                          (capi.PLAN_AUTO, keep[3:]), (capi.PLAN_STAGEWISE, keep[1:])):
            got = capi.synth(d, [pop.staged[k] for k in ks], flags=flags, mform=flags == capi.PLAN_LEAN_ALWAYS)
            for k, g in zip(ks, got):
                assert np.array_equal(g, pop.want[k][0]), (flags, k)


# ---------------------------------------------------------------------------------------------------------------- the device parser's arena contract

@pytest.mark.parametrize("ranges", [1, 3])
def test_device_parser_int16_arena_contract(pop, ranges):
    """ACM_BATCH_STAGE_INT16, device parsing: D_IDX and D_HDR after the call against the host stager, and the fill outside the slices.  The
    truncated and the H1 stream are flagged by the walk and staged again by the host reader (tests/test_gpu_damaged_streams.py): their
    slices hold the host's staging over the blocks it staged"""
    flags = capi.BATCH_STAGE_INT16 | capi.batch_ranges(ranges)
    lay = layout(pop, flags, 0, capi.PARSE_DEVICE)
    assert lay["totals"]["dev_parse"] and not lay["totals"]["dev_mform"]
    with capi.Device(0) as d:
        res, tm = capi.batch_decode(d, pop.files, parse=capi.PARSE_DEVICE, threads=4, byteplane=False, batch_flags=capi.batch_ranges(ranges))
        check_batch(pop, res, ranges)
        print("R %d  device_parsed %d  host_parsed %d" % (lay["totals"]["R"], tm.device_parsed, tm.host_parsed))
        assert tm.device_parsed == len(pop.files) - 3 and tm.host_parsed == 2
        d_idx, d_hdr = read_arena(d, "D_IDX", np.int16), read_arena(d, "D_HDR", np.uint32).reshape(-1, 2)
    assert d_idx.size == max(lay["totals"]["idx_total"], 8)
    inside = check_int16_arenas(pop, lay, d_idx, d_hdr, dirty_too=True)
    assert (~inside).sum() > 0
    dirty = np.nonzero(~inside & (d_idx != IDX_FILL))[0]
    assert dirty.size == 0, "%d indices written outside the streams' slices, the first at %d" % (dirty.size, dirty[0])


@pytest.mark.parametrize("ranges", [1, 3])
def test_device_parser_byteplane_arena_contract(pop, ranges):
    """default staging, device parsing: the streams of the chunk kernel's levels are written in the byte-plane form by the column kernel.
    The device parser has no 12-bit class, so the comparison goes through the inverse: acmhip_mform_unrows over the device's blob and pair
    table gives the staged indices of rows [0, mf_rows) back; the int16 arena holds the rows from mf_rows - 2 on and the fill in front of
    them; pair-table entries and blob bytes that belong to no stream - and a clean stream's bytes behind its last pair - keep the fill"""
    L = capi.lib()
    lay = layout(pop, capi.batch_ranges(ranges), capi.PLAN_LEAN_ALWAYS, capi.PARSE_DEVICE)
    tot = lay["totals"]
    assert tot["dev_parse"] and tot["dev_mform"]
    with capi.Device(0) as d:
        res, tm = capi.batch_decode(d, pop.files, parse=capi.PARSE_DEVICE, threads=4, flags=capi.PLAN_LEAN_ALWAYS, batch_flags=capi.batch_ranges(ranges))
        check_batch(pop, res, ranges)
        print("R %d  device_parsed %d  host_parsed %d  packed_streams %d" % (tot["R"], tm.device_parsed, tm.host_parsed, tm.packed_streams))
        assert tm.device_parsed == len(pop.files) - 3
        d_idx, d_hdr = read_arena(d, "D_IDX", np.int16), read_arena(d, "D_HDR", np.uint32).reshape(-1, 2)
        blob, pairs = read_arena(d, "D_PKBLOB", np.uint8), read_arena(d, "D_PKCHUNK", np.uint32)
    assert pairs.size == tot["mf_pairs_total"] + 32 and blob.size == tot["mf_total"] + (128 << 10)
    first_row = [0] * len(pop.files)
    # a stream's reservation in the blob arena and in the pair table: from its offset to the next stream's (the layout places them in order)
    holders = sorted((int(sl["mf_off"]), int(sl["mf_pair_off"]), k) for k, sl in enumerate(lay["slots"]) if sl["ok"] and sl["mf_rows_cap"])
    ends = {k: (nb, npo) for (_, _, k), (nb, npo, _) in zip(holders, holders[1:] + [(tot["mf_total"], tot["mf_pairs_total"], None)])}
    assert holders and holders[0][:2] == (0, 0) and all(a[:2] < b[:2] for a, b in zip(holders, holders[1:]))
    classes, odd_pairs, formed = set(), 0, 0
    mf_rows = {int(k): int(job["mf_rows"]) for k, job in zip(lay["dev_ids"], lay["jobs"])}
    for bo, po, k in holders:
        s, rows = pop.staged[k], mf_rows[k]
        level, cols = s.info.level, s.info.cols
        end_b, end_p = ends[k]
        if not pop.clean(k):
            continue                    # flagged by the walk: its entries are parked, the host reader staged it as int16
        if not rows:                    # room in the arenas, but no whole tile in the end: nobody writes there
            assert (blob[bo:end_b] == 0).all() and (pairs[po:end_p] == 0).all(), k
            continue
        job = lay["jobs"][list(lay["dev_ids"]).index(k)]
        assert bo == int(job["mf_off"]) and po == int(job["mf_pair_off"]) and rows % 2 == 0 and bo % 64 == 0
        assert L.acmk_tile2m_stages(level) == 6 and rows <= int(lay["slots"][k]["mf_rows_cap"]) and po + rows // 2 + 1 <= end_p
        formed += 1
        first_row[k] = rows - 2
        mine = pairs[po:po + rows // 2 + 1]
        got = capi.mform_unrows(level, blob, mine, rows)
        bad = np.nonzero(got != s.idx[:rows * cols])[0]
        assert bad.size == 0, "stream %d (level %d, %d rows a block): %d indices of the byte-plane rows differ, first at row %d" % (
            k, level, s.info.rows, bad.size, bad[0] // cols)
        # the pairs lie back to back from the pair of zeros on, each at the class its blocks' pwr asks for; nothing behind the last one
        at = bo // 64
        assert int(mine[0]) == (at << 2 | 2), k
        at += 2 * cols // 64
        for p in range(rows // 2):
            cls = int(mine[p + 1]) & 3
            assert int(mine[p + 1]) >> 2 == at, (k, p)
            b0, b1 = (2 * p) // s.info.rows, (2 * p + 1) // s.info.rows
            want_cls = max((2 if int(s.hdr[b, 1]) < 8 else 0 if int(s.hdr[b, 1]) == 15 else 3 for b in (b0, b1)), key=lambda c: (2, 3, 0).index(c))
            assert cls == want_cls, (k, p, cls, want_cls)
            classes.add(cls)
            odd_pairs += b0 != b1
            at += cols * HALF_BYTES[cls] // 64
        assert at * 64 <= end_b, k
        tail = blob[at * 64:end_b]
        assert (tail == 0).all(), "stream %d: %d bytes written behind its last pair" % (k, int((tail != 0).sum()))
        assert (pairs[po + rows // 2 + 1:end_p] == 0).all(), "stream %d: pair-table entries written behind its last pair" % k
    print("streams in the form %d  classes %s  pairs across two blocks %d" % (formed, sorted(classes), odd_pairs))
    assert formed >= 12 and classes == {0, 2, 3} and odd_pairs > 0
    assert (pairs[tot["mf_pairs_total"]:] == 0).all() and pairs.size - tot["mf_pairs_total"] == 32, "pair-table entries of no stream were written"
    assert (blob[tot["mf_total"]:] == 0).all() and blob.size - tot["mf_total"] == 128 << 10, "byte-plane bytes of no stream were written"
    inside = check_int16_arenas(pop, lay, d_idx, d_hdr, dirty_too=True, first_row=first_row)
    dirty = np.nonzero(~inside & (d_idx != IDX_FILL))[0]
    assert dirty.size == 0, "%d indices written outside the streams' slices, the first at %d" % (dirty.size, dirty[0])


# ---------------------------------------------------------------------------------------------------------------- orders the suite never ran

def test_orders_the_suite_only_ran_one_way(pop):
    """one fresh handle, mode on, every call against the oracle: device parsing BEFORE host parsing, 3 block ranges before 1, byte planes
    before int16 staging, float32 before int16 output"""
    lean = capi.PLAN_LEAN_ALWAYS
    with capi.Device(0) as d:
        for kw in (dict(parse=capi.PARSE_DEVICE, flags=lean, batch_flags=capi.batch_ranges(3)),
                   dict(parse=capi.PARSE_DEVICE, flags=lean, batch_flags=capi.batch_ranges(1)),
                   dict(parse=capi.PARSE_HOST, flags=lean),
                   dict(parse=capi.PARSE_HOST, flags=lean, byteplane=False),
                   dict(parse=capi.PARSE_DEVICE, byteplane=True, batch_flags=capi.batch_ranges(3)),
                   dict(parse=capi.PARSE_DEVICE, byteplane=False, batch_flags=capi.batch_ranges(3)),
                   dict(parse=capi.PARSE_DEVICE, byteplane=False, batch_flags=capi.batch_ranges(1))):
            res, tm = capi.batch_decode(d, pop.files, threads=4, **kw)
            check_batch(pop, res, kw)
            assert (tm.device_parsed > 0) == (kw["parse"] == capi.PARSE_DEVICE)
        assert d.fill
        cap = capi.batch_pcm_words(pop.files)
        d_pcm = d.malloc(cap * 4)
        try:
            for f32 in (True, False):
                d.memset(d_pcm, 0xFF if f32 else 0xA5, cap * 4)
                st, words, offs, tm = capi.batch_decode_device(d, pop.files, d_pcm, cap, threads=4, parse=capi.PARSE_DEVICE, f32=f32, flags=lean)
                got = np.zeros(cap, np.uint32 if f32 else np.uint16)
                d.download(got, d_pcm)
                written = np.zeros(cap, bool)
                for k, (want, wst) in enumerate(pop.want):
                    if k == pop.not_acm:
                        assert st[k] != 0 and words[k] == 0
                        continue
                    a, b = offs[k], offs[k] + words[k]
                    assert st[k] == wst and words[k] == want.size and not written[a:b].any(), (f32, k)
                    written[a:b] = True
                    if f32:
                        assert np.array_equal(got[a:b].view(np.float32), want.view(np.int16).astype(np.float32) * np.float32(2.0 ** -15)), k
                    else:
                        assert np.array_equal(got[a:b], want), k
                assert (got[~written] == (capi.POISON32 if f32 else capi.POISON16)).all(), f32
        finally:
            d.free(d_pcm)


# ---------------------------------------------------------------------------------------------------------------- capi.synth poisons

@pytest.mark.parametrize("f32", [False, True], ids=["s16le", "float32"])
def test_synth_poisons_its_pcm_buffer(pop, f32):
    """a synth of streams A, then one over the same arena layout whose descriptor list leaves a stream out: the slot of that stream reads
    back as poison, word for word - not as the PCM the first call left in the buffer the allocator hands out again"""
    ks = [k for k in range(len(pop.files)) if k != pop.not_acm][:24]
    staged = [pop.staged[k] for k in ks]
    out = 22                                    # level 9, 16 rows: a stream of the lean kernels in the middle of the arena
    with capi.Device(0) as d:
        for omit in ((), (out,), ()):
            got = capi.synth(d, staged, f32=f32, omit=omit)
            for j, (k, g) in enumerate(zip(ks, got)):
                want = pop.want[k][0]
                assert g.size == want.size > 0
                if j in omit:
                    assert (g.view(np.uint32) == capi.POISON32).all() if f32 else (g == capi.POISON16).all(), "the slot of the stream left out holds something"
                elif f32:
                    assert np.array_equal(g, want.view(np.int16).astype(np.float32) * np.float32(2.0 ** -15)), k
                else:
                    assert np.array_equal(g, want), k
