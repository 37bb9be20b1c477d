"""The public host stagers held to fingerprints recorded from an EARLIER commit (tests/golden/stagers.json, written by
tests/golden/make_golden_stagers.py): acm_stage_probe, acm_index_file, acm_stage_file, acm_stage_file_mform, acm_stage_window and the
test hook acmk_stage_marks (libacm_amd/csrc/acm_stage.cpp).  No device.

Every output buffer is handed over full of POISON bytes, with PAD entries more than the call may fill, and hashed WHOLE (sha256): a
store outside what the recorded commit wrote shows, and so does one it made and this tree does not - the rows a failing block leaves
half written, the pairs a byte-plane attempt wrote before it fell back.  The return code, every field of acm_stage_info (poisoned too:
a call that refuses its arguments leaves it alone), mf_rows and mf_bytes are recorded beside the digests.

build_cases() and run_case() are all the generator and this test do, so the test cannot drift from what was recorded; the test calls
nothing but the library under test and compares with the JSON.  The files are a few blocks each (helpers.make_stream): the smallest
shapes at which each branch of the stagers is taken."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN_DIR, make_stream
from libacm_amd import capi

FIXTURE = os.path.join(GOLDEN_DIR, "stagers.json")
POISON = 0xA5
PAD = 3                 # entries behind what a call may fill, in every buffer
CALLS = ("probe", "index", "file", "mform", "window", "marks")
LEVELS = (0, 2, 5, 6, 7, 8, 9, 11, 12, 13, 14)
INFO_FIELDS = [f for f, _ in capi.StageInfo._fields_]
MARK, PATCH, HDR = capi.BLOCK_MARK_DT.itemsize, 16, 8          # bytes per acm_block_mark, acmhip_patch, acmhip_blkhdr


class File:
    """a file image and what its header says, from the parameters it was written with (buffers are sized by these, not by the library)"""

    def __init__(self, name, data, level, rows, promised):
        self.name, self.data, self.level, self.rows, self.promised = name, bytes(data), level, rows, promised
        self.bl = rows << level

    def cut(self, n):
        return File("%s[:%d]" % (self.name, n), self.data[:n], self.level, self.rows, self.promised)


def stream(name, seed, level, rows, nblocks, channels=1, cut=0, **kw):
    promised = -(-max(1, nblocks * (rows << level) - cut) // (rows << level))
    return File(name, make_stream(seed, level, rows, nblocks, channels=channels, cut=cut, **kw), level, rows, promised)


def h1_stream(level):
    return stream("h1_L%d" % level, 9100 + level, level, 16, 6, allow_out_of_range=1, pwr_min=0, pwr_max=3)


def form_blocks(level, rows):
    """a few blocks; at a level with the byte-plane form enough of them for a whole tile of the lean kernel and a ragged tail behind it"""
    L = capi.lib()
    t2 = L.acmk_tile2_rows(level)
    return max(3, -(-(t2 + 3) // rows)) if L.acmhip_mform_tile_rows(level) > 0 and level <= 12 else 3


def poisoned(nbytes):
    return np.full(max(int(nbytes), 1), POISON, dtype=np.uint8)


def sha(buf):
    return hashlib.sha256(buf.tobytes()).hexdigest()


def stagers_of(level):
    L = capi.lib()
    return [0] + ([1] if L.acmhip_mform_tile_rows(level) > 0 else []) + ([2] if L.acmhip_packed_tile_rows(level) > 0 else [])


def own_marks(f, force_chans=0):
    """acm_index_file's marks[0 .. blocks] of a file, as BLOCK_MARK_DT records"""
    a = capi._as_u8(f.data)
    marks = np.zeros(f.promised + 1, dtype=capi.BLOCK_MARK_DT)
    info = capi.StageInfo()
    assert capi.lib().acm_index_file(a.ctypes.data, a.size, force_chans, marks.ctypes.data, f.promised, C.byref(info)) == 0
    return marks[:info.blocks + 1].copy()


def npatches_of(f):
    a = capi._as_u8(f.data)
    info = capi.StageInfo()
    idx, hdr = poisoned(2 * f.promised * f.bl), poisoned(HDR * f.promised)
    assert capi.lib().acm_stage_file(a.ctypes.data, a.size, 0, idx.ctypes.data, hdr.ctypes.data, f.promised, None, 0, C.byref(info)) == 0
    return int(info.npatches)


# --------------------------------------------------------------------------- the cases
def case(call, f, **args):
    tag = ",".join("%s=%s" % (k, v) for k, v in sorted(args.items()) if k not in ("marks",))
    return dict(args, call=call, file=f, id="%s:%s:%s" % (call, f.name, tag))


def whole_file_cases(f, force_chans=0, max_blocks=None, marks_too=True):
    """one file through every call that takes a whole file"""
    mb = f.promised if max_blocks is None else max_blocks
    out = [case("probe", f, force_chans=force_chans), case("index", f, force_chans=force_chans, max_blocks=mb),
           case("file", f, force_chans=force_chans, max_blocks=mb, max_patches=0), case("mform", f, force_chans=force_chans, max_blocks=mb)]
    if marks_too:
        out += [case("marks", f, force_chans=force_chans, max_blocks=mb, stager=s) for s in stagers_of(f.level)]
    return out


def window_cases(f, marks, nidx, firsts, tag, max_patches=0):
    return [case("window", f, marks=marks, marks_of=tag, nidx=nidx, first=first, count=count, max_patches=max_patches)
            for first in firsts for count in (2, 9)]


def build_cases():
    cases = []
    # levels and block heights (odd heights: the byte-plane stager's straddle row)
    for level in LEVELS:
        for rows in ((1, 2, 3, 16, 17) if level < 13 else (2, 3)):
            cases += whole_file_cases(stream("L%d_r%d" % (level, rows), 9000 + 20 * level + rows, level, rows, form_blocks(level, rows)))
    # headers: two channels with a cut (total_values is not a whole block), a WAVC prefix, forced channel counts
    for level in (2, 7):
        stereo = stream("stereo_L%d" % level, 9400 + level, level, 16, 6, channels=2, cut=5)
        wavc = stream("wavc_L%d" % level, 9410 + level, level, 16, 6, wavc=1)
        mono = stream("mono_L%d" % level, 9420 + level, level, 16, 6, cut=1)
        for f in (stereo, wavc, mono):
            for fc in (-1, 0, 2):
                cases += whole_file_cases(f, force_chans=fc)
    # H1: indices outside the block's amplitude range, with no room for the patches, one short, and ample
    for level in (3, 7, 9):
        f = h1_stream(level)
        cases += whole_file_cases(f)
        cases += [case("file", f, force_chans=0, max_blocks=f.promised, max_patches=mp) for mp in ("found-1", "found+3")]
    # max_blocks below, at and above what the header promises
    for f in (stream("mb_L7", 9500, 7, 16, 6), stream("mb_L2", 9501, 2, 3, 6), h1_stream(7)):
        for mb in (0, 3, 6, 8):
            cases += whole_file_cases(f, max_blocks=mb)
    # a file that ends early, cut around the first byte of every block and one byte short of its end
    whole = stream("cut_L7", 860, 7, 16, 6)
    bits = [int(m["bit"]) for m in own_marks(whole)]
    for n in sorted({b // 8 + d for b in bits[:-1] for d in (-1, 0, 1)} | {len(whole.data) - 1}):
        cases += whole_file_cases(whole.cut(n))
    # short files and a file that is not ACM
    small = stream("small_L5", 870, 5, 4, 3)
    foreign = File("not_acm", b"RIFF this is not an acm file at all", 5, 4, 3)
    for f in (small.cut(0), small.cut(13), small.cut(14), small.cut(19), foreign):
        cases += whole_file_cases(f, marks_too=False)
        cases += [case("marks", f, force_chans=0, max_blocks=f.promised, stager=s) for s in (0, 1, 2)]
        cases += window_cases(f, own_marks(small), 3, (0, 1), "small")
    # windows through the file's own index - whole, and one that ends in the middle of the file, entered through its last block -
    win, h1 = stream("win_L7", 9600, 7, 16, 6), h1_stream(7)
    for f in (win, h1):
        marks = own_marks(f)
        assert len(marks) == 7
        found = npatches_of(f)
        cases += window_cases(f, marks, 6, (0, 1, 3, 6, 7), "own", max_patches=found + 3)
        cases += window_cases(f, marks[:4].copy(), 3, (0, 1, 2, 3, 4), "own", max_patches=found + 3)
        cases += window_cases(f, marks, 6, (1, 3), "own", max_patches=0)
    # ... through the index of another file, and through marks one bit off
    other = own_marks(stream("other_L7", 9601, 7, 16, 6))
    shifted = own_marks(win)
    shifted["bit"] += 1
    one_off = own_marks(win)
    one_off["bit"][3] += 1
    for marks, tag in ((other, "other"), (shifted, "shifted"), (one_off, "mark3+1")):
        cases += window_cases(win, marks, 6, (0, 1, 3, 6), tag)
    return list({c["id"]: c for c in cases}.values())          # (an id says everything about a call: the same call asked for twice runs once)


# --------------------------------------------------------------------------- one call
def run_case(c):
    """-> {"rc", "info", "sha": {buffer: sha256 of the whole buffer}, ...}: everything the call hands back"""
    L = capi.lib()
    f = c["file"]
    a = capi._as_u8(f.data)
    info = capi.StageInfo()
    C.memset(C.byref(info), POISON, C.sizeof(info))
    bufs, out = {}, {}

    def buf(name, nbytes):
        bufs[name] = poisoned(nbytes)
        return bufs[name].ctypes.data

    fc = c.get("force_chans", 0)
    mb = c.get("max_blocks", 0)
    if c["call"] == "probe":
        rc = L.acm_stage_probe(a.ctypes.data, a.size, fc, C.byref(info))
    elif c["call"] == "index":
        rc = L.acm_index_file(a.ctypes.data, a.size, fc, buf("marks", MARK * (mb + 1 + PAD)), mb, C.byref(info))
    elif c["call"] == "file":
        mp = c["max_patches"]
        if isinstance(mp, str):                 # relative to what the stream holds
            mp = out["max_patches"] = max(0, npatches_of(f) + int(mp[len("found"):]))
        rc = L.acm_stage_file(a.ctypes.data, a.size, fc, buf("idx", 2 * (mb * f.bl + PAD)), buf("hdr", HDR * (mb + PAD)), mb,
                              buf("patches", PATCH * (mp + PAD)), mp, C.byref(info))
    elif c["call"] == "mform":
        nrows = (mb * f.rows) & ~1
        rows, nbytes = C.c_uint64(0xA5A5A5A5A5A5A5A5), C.c_uint64(0xA5A5A5A5A5A5A5A5)
        rc = L.acm_stage_file_mform(a.ctypes.data, a.size, fc, buf("idx", 2 * (mb * f.bl + PAD)), buf("hdr", HDR * (mb + PAD)), mb, C.byref(info),
                                    buf("blob", int(L.acmhip_mform_bytes(f.level, nrows)) + 256), 0,
                                    buf("pairs", 4 * (int(L.acmhip_mform_pairs(nrows)) + 32)), C.byref(rows), C.byref(nbytes))
        out["mf_rows"], out["mf_bytes"] = rows.value, nbytes.value
    elif c["call"] == "window":
        marks = np.ascontiguousarray(c["marks"], dtype=capi.BLOCK_MARK_DT)
        assert marks.size >= c["nidx"] + 1
        rc = L.acm_stage_window(a.ctypes.data, a.size, fc, marks.ctypes.data, c["nidx"], c["first"], c["count"],
                                buf("idx", 2 * (c["count"] * f.bl + PAD)), buf("hdr", HDR * (c["count"] + PAD)),
                                buf("patches", PATCH * (c["max_patches"] + PAD)), c["max_patches"], C.byref(info))
    else:
        fn = L.acmk_stage_marks
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(capi.StageInfo)]
        rc = fn(a.ctypes.data, a.size, fc, c["stager"], buf("marks", MARK * (mb + 1 + PAD)), mb, C.byref(info))
    out.update(rc=int(rc), info=[int(getattr(info, k)) for k in INFO_FIELDS], sha={k: sha(v) for k, v in bufs.items()},
               untouched=sorted(k for k, v in bufs.items() if np.all(v == POISON)))
    return out


def record():
    """every case through the library that is loaded -> {id: result}"""
    return {c["id"]: run_case(c) for c in build_cases()}


# --------------------------------------------------------------------------- the test
_got = None


@pytest.mark.parametrize("call", CALLS)
def test_stagers_match_the_recorded_commit(call):
    global _got
    with open(FIXTURE) as fh:
        want = json.load(fh)["cases"]
    if _got is None:
        _got = record()
    assert sorted(_got) == sorted(want), "the case list is not the recorded one"
    ids = [i for i in want if i.startswith(call + ":")]
    assert ids
    wrong = [i for i in ids if _got[i] != want[i]]
    assert not wrong, "%d of %d %s cases differ from the recorded commit, e.g. %s: got %s, recorded %s" % (
        len(wrong), len(ids), call, wrong[0], _got[wrong[0]], want[wrong[0]])
