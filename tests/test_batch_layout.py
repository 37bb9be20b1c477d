"""The batch front end's device-free half (libacm_amd/csrc/acm_batch_layout.cpp), without a GPU.

acmk_batch_layout_visit() computes the layout of a batch from probed headers, file lengths and options alone and shows every table of
it.  Three kinds of check over one list of cases:

  * equality: the SHA-256 of every table and of the totals record (every total, every mode decision, the return code) equals what
    acm_batch_decode of the commit named in tests/golden/batch_layout.json computed for the same case (recorded from that commit's own
    lines by tests/golden/make_golden_batch_layout.py through the dry-run seam in profiles/batch_layout_parent_seam.patch);
  * coverage: the case list reaches both sides of every decision the layout takes (a condition on the list, asserted by the recorder on
    the recorded code's output and here again);
  * properties of the tables themselves: arena slices are disjoint and aligned, chunks tile the arenas, the pieces of the block ranges
    add up to what every stream delivers, the stripes tile the file arena, byte-plane rows are whole tiles, every live stream has a parser.

A case is a list of streams (level, rows, total_values, channels, header_bytes, len, ok, has_pcm) and the options; nothing is allocated
beyond the tables, so shapes of any size cost nothing.
"""
import ctypes as C
import hashlib
import itertools
import json
import os

import numpy as np

from libacm_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_layout.json")

TABLE_NAMES = ("slots", "chunks", "groups", "dev_ids", "host_ids", "out_ids", "jobs", "piece_off", "piece_len", "rbase", "stripe_at",
               "stripe_base")
SLOT = np.dtype([(f, "<u8") for f in ("need_blocks", "idx_off", "hdr_off", "pcm_off", "idx_len", "chunk", "pk_chunk_off", "pk_chunk_cap",
                                      "pk_ntiles", "mf_off", "mf_rows_cap", "mf_pair_off", "range_unit", "file_off", "on_dev", "ok")])
CHUNK = np.dtype([(f, "<u8") for f in ("first", "last", "idx_begin", "idx_end", "hdr_begin", "hdr_end", "pk_chunk_begin", "pk_chunk_end",
                                       "mf_begin", "mf_end", "mf_pair_begin", "mf_pair_end")])
GROUP = np.dtype([(f, "<u8") for f in ("k_first", "k_last", "file_begin", "file_end", "max_columns")])
JOB = np.dtype([("file_off", "<u8"), ("idx_off", "<u8"), ("hdr_off", "<u8"), ("col_off", "<u8"), ("file_len", "<u4"), ("data_start", "<u4"),
                ("level", "<u4"), ("rows", "<u4"), ("blocks", "<u4"), ("range_unit", "<u4"), ("mf_off", "<u8"), ("mf_pair_off", "<u4"),
                ("mf_rows", "<u4")])
DTYPES = dict({"slots": SLOT, "chunks": CHUNK, "groups": GROUP, "jobs": JOB}, **{t: "<u8" for t in TABLE_NAMES[3:6] + TABLE_NAMES[7:]})
TOTALS = ("idx_total", "hdr_total", "pcm_total", "pcm_arena_words", "pk_chunks_total", "mf_total", "mf_pairs_total", "files_total",
          "cols_total", "jobs_bytes", "res_bytes", "stripe_tab_off", "stripe_tab_bytes", "R", "stage_packed", "stage_mform", "dev_parse",
          "dev_mform", "direct_out", "keep_on_device", "rc")
RANGE_MAX_STREAMS = 32768       # ACM_PARSE_RANGE_MAX_STREAMS

VISIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_size_t)


def _lib():
    L = capi.lib()
    L.acmk_batch_layout_visit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int,
                                          VISIT, C.c_void_p]
    for f in ("acmk_tile2_rows", "acmk_tile2m_rows", "acmk_tile2m_stages", "acmhip_mform_tile_rows"):
        getattr(L, f).restype = C.c_int
        getattr(L, f).argtypes = [C.c_uint32]
    return L


# ---------------------------------------------------------------------------------------------------------------- the case list

class Case:
    """streams: (level, rows, total_values, channels, header_bytes, len, ok, has_pcm)"""

    def __init__(self, name, streams, flags=0, plan_flags=0, parse=capi.PARSE_HOST, threads=4, d_pcm_words=None, prestaged=False):
        self.name, self.streams, self.flags, self.plan_flags, self.parse = name, streams, flags, plan_flags, parse
        self.threads, self.d_pcm_words, self.prestaged = threads, d_pcm_words, prestaged


def stream(level, rows, blocks, channels=1, short_by=0, bits_per_sample=6, header_bytes=14, ok=1, has_pcm=1, length=None):
    """a stream of `blocks` blocks whose last one is `short_by` samples short, in a file of a plausible length"""
    bl = rows << level
    total = max(blocks * bl - short_by, 1)
    if length is None:
        length = header_bytes + (blocks * (20 + bl * bits_per_sample) + 7) // 8 + 3
    return (level, rows, total, channels, header_bytes, length, ok, has_pcm)


def mix41():
    """the batch of tests/test_gpu_parity.py::test_batch_block_ranges as headers: levels 0-13, rows 1 / 3 / 16 / 33, 1-23 blocks, mono and
    stereo, ragged ends, a truncated file, something that is not ACM in the middle"""
    out = []
    for i in range(41):
        lv, rows, nb = [7, 9, 5, 3, 11, 0, 13, 8][i % 8], [16, 3, 1, 33][i % 4], 1 + (i * 7) % 23
        out.append(stream(lv, rows, nb, channels=1 + i % 2, short_by=(i % 5) * ((rows << lv) // 7 + 1)))
    out[6] = out[6][:5] + (out[6][5] * 2 // 3,) + out[6][6:]
    out[13] = (0, 0, 0, 0, 0, 8, 0, 1)
    return out


STAGINGS = {"default": 0, "int16": capi.BATCH_STAGE_INT16, "packed": capi.BATCH_STAGE_PACKED, "byteplane": capi.BATCH_STAGE_BYTEPLANE,
            "packed_byteplane": capi.BATCH_STAGE_PACKED | capi.BATCH_STAGE_BYTEPLANE}
PLAN_FLAGS = {"auto": 0, "no_lean": capi.PLAN_NO_LEAN, "stagewise": capi.PLAN_STAGEWISE}
PARSES = {"host": (capi.PARSE_HOST, 4), "device": (capi.PARSE_DEVICE, 4), "auto1": (capi.PARSE_AUTO, 1), "auto4": (capi.PARSE_AUTO, 4),
          "auto64": (capi.PARSE_AUTO, 64)}
RANGES = (0, 1, 2, 3, 8, 16, 64)
OUTPUTS = ("host", "device", "pinned")


def build_cases(L):
    cases = [Case("empty", []), Case("nothing_decodable", [(0, 0, 0, 0, 0, 8, 0, 1), (0, 0, 0, 0, 0, 0, 0, 0)]),
             Case("nothing_decodable_device", [(0, 0, 0, 0, 0, 8, 0, 1)], parse=capi.PARSE_DEVICE)]
    for parse in ("host", "device"):
        for r in (0, 4):
            cases.append(Case("single_%s_r%d" % (parse, r), [stream(9, 16, 40)], flags=capi.batch_ranges(r), parse=PARSES[parse][0]))
    mix = mix41()
    mix_words = sum(-(-(s[2]) // 64) * 64 for s in mix if s[6]) + 64 * 41
    for st, pre, pf, parse, r, out in itertools.product(STAGINGS, (False, True), PLAN_FLAGS, PARSES, RANGES, OUTPUTS):
        cases.append(Case("mix41_%s_%s_%s_%s_r%d_%s" % (st, "pre" if pre else "files", pf, parse, r, out), mix,
                          flags=STAGINGS[st] | capi.batch_ranges(r) | (capi.BATCH_PCM_PINNED if out == "pinned" else 0),
                          plan_flags=PLAN_FLAGS[pf], parse=PARSES[parse][0], threads=PARSES[parse][1],
                          d_pcm_words=4 * mix_words if out == "device" else None, prestaged=pre))
    cases.append(Case("mix41_d_pcm_too_small", mix, d_pcm_words=1000))
    # pinned output below the 32768-words-per-stream line (the mix is above it), and nobody wants the PCM
    small = [stream(7, 4, 1 + k % 5, short_by=k) for k in range(20)]
    cases.append(Case("small_pinned", small, flags=capi.BATCH_PCM_PINNED))
    cases.append(Case("mix41_no_pcm", [s[:7] + (0,) for s in mix], parse=capi.PARSE_DEVICE, flags=capi.batch_ranges(3)))
    # block ranges at the chunk kernel's levels: block heights that share no factor with the tile (range_unit > 1), blocks that are
    # whole tiles (range_unit == 1), and a level without the form beside them
    odd = []
    for lv in range(5, 15):
        t2 = L.acmk_tile2_rows(lv) or 4
        odd += [stream(lv, rows, nb, channels=1 + nb % 2, short_by=nb) for rows, nb in ((3, 37), (t2, 5), (2 * t2, 3), (t2 + 1, 9), (1, 64))]
    for r in (2, 5, 16):
        for st in ("default", "int16"):
            cases.append(Case("tiles_%s_r%d" % (st, r), odd, flags=STAGINGS[st] | capi.batch_ranges(r), parse=capi.PARSE_DEVICE))
    cases.append(Case("tiles_host", odd))
    # a file too short for what its header promises: the arenas are sized by what the file can hold
    short = [stream(9, 16, 1000, length=14 + 400), stream(7, 1, 1 << 20, length=19), stream(9, 16, 3), stream(5, 2, 77, length=14)]
    for parse in ("host", "device"):
        cases.append(Case("short_files_" + parse, short, parse=PARSES[parse][0], flags=capi.batch_ranges(2)))
    # a stream the device parser refuses (256 MiB of file) among ones it takes: both parsers have work, no ranges
    refused = [stream(9, 16, 20), stream(9, 16, 30, length=1 << 28), stream(11, 4, 9), stream(3, 2, 5)]
    for r in (0, 4):
        cases.append(Case("refused_r%d" % r, refused, parse=capi.PARSE_DEVICE, flags=capi.batch_ranges(r)))
    # many chunks; AUTO on both sides of its threshold
    many = [stream(9, 16, 12, channels=1 + k % 2, short_by=k) for k in range(96)]
    for parse in PARSES:
        for st in ("default", "packed", "int16"):
            cases.append(Case("many_%s_%s" % (parse, st), many, flags=STAGINGS[st], parse=PARSES[parse][0], threads=PARSES[parse][1]))
    # the headline batch: reaches the automatic range count
    headline = [stream(9, 16, 250)] * 1024
    for parse in ("host", "auto4", "auto64", "device"):
        cases.append(Case("headline_" + parse, headline, parse=PARSES[parse][0], threads=PARSES[parse][1]))
    cases.append(Case("headline_device_pinned", headline, parse=capi.PARSE_DEVICE, flags=capi.BATCH_PCM_PINNED))
    cases.append(Case("headline_host_pinned", headline, flags=capi.BATCH_PCM_PINNED))
    cases.append(Case("headline_device_r1", headline, parse=capi.PARSE_DEVICE, flags=capi.batch_ranges(1)))
    # more streams than the range walk takes
    crowd = [stream(7, 8, 2, short_by=k % 3) for k in range(33000)]
    for st in ("default", "int16"):
        cases.append(Case("crowd_device_r4_" + st, crowd, parse=capi.PARSE_DEVICE, flags=STAGINGS[st] | capi.batch_ranges(4)))
    cases.append(Case("crowd_auto64", crowd, parse=capi.PARSE_AUTO, threads=64))
    cases.append(Case("crowd_edge_device_r4", crowd[:RANGE_MAX_STREAMS], parse=capi.PARSE_DEVICE, flags=capi.batch_ranges(4)))
    # a byte-plane arena past 2^36 bytes: the form is dropped
    huge = [(9, 16, 0xFFFFFFFF, 1, 14, 200 << 20, 1, 0)] * 24
    for parse in ("host", "device"):
        cases.append(Case("huge_" + parse, huge, parse=PARSES[parse][0]))
    cases.append(Case("huge_half", huge[:6]))
    # levels no second form covers: the batch travels as int16 whatever is asked
    low = [stream(lv, rows, 9, short_by=lv) for lv in (0, 3, 5) for rows in (1, 4, 33)]
    for st in ("default", "packed"):
        for parse in ("host", "device"):
            cases.append(Case("low_%s_%s" % (st, parse), low, flags=STAGINGS[st], parse=PARSES[parse][0]))
    return cases


# ---------------------------------------------------------------------------------------------------------------- running, recording

def run_case(L, case):
    """{"rc", "tables": {name: bytes}, "elem": {name: elem_bytes}} in visiting order"""
    n = len(case.streams)
    info = (capi.StageInfo * max(n, 1))()
    length, ok, has_pcm = (C.c_uint64 * max(n, 1))(), (C.c_uint8 * max(n, 1))(), (C.c_uint8 * max(n, 1))()
    for k, (level, rows, total, channels, header_bytes, ln, good, pcm) in enumerate(case.streams):
        info[k] = capi.StageInfo(level, rows, 1 << level, channels, channels, 22050, total, 0, 0, 0, 0, header_bytes)
        length[k], ok[k], has_pcm[k] = ln, good, pcm
    opts = capi.BatchOpts(0, 0, case.threads, case.plan_flags, case.parse, case.flags, 0x100 if case.d_pcm_words is not None else None,
                          case.d_pcm_words or 0, None)
    tables, elem = {}, {}

    def visit(_ctx, name, data, elem_bytes, count):
        name = name.decode()
        assert name not in tables
        tables[name] = C.string_at(data, elem_bytes * count)
        elem[name] = elem_bytes
    cb = VISIT(visit)
    rc = L.acmk_batch_layout_visit(info, length, ok, has_pcm, n, C.byref(opts), case.threads, int(case.prestaged), cb, None)
    return {"rc": rc, "tables": tables, "elem": elem}


def digest(case, res):
    h = hashlib.sha256(("%s rc=%d" % (case.name, res["rc"])).encode())
    for name, raw in res["tables"].items():
        h.update(("|%s:%d:%d|" % (name, res["elem"][name], len(raw))).encode())
        h.update(raw)
    return h.hexdigest()


def recording(cases, results):
    each = [digest(c, r) for c, r in zip(cases, results)]
    return {"sha256_of_all": hashlib.sha256("".join(each).encode()).hexdigest(),
            "errors": {c.name: r["rc"] for c, r in zip(cases, results) if r["rc"] != 0}, "case_sha256_16": [e[:16] for e in each]}


def decode(res):
    out = {name: np.frombuffer(raw, dtype=DTYPES[name]) for name, raw in res["tables"].items() if name != "totals"}
    if "totals" in res["tables"]:
        words = np.frombuffer(res["tables"]["totals"], dtype="<u8")
        assert len(words) == len(TOTALS)
        out["totals"] = {k: int(v) for k, v in zip(TOTALS, words)}
    return out


# ---------------------------------------------------------------------------------------------------------------- coverage

def coverage(cases, results):
    """what the case list reaches, as {condition: bool}; every one must hold"""
    seen = {}

    def mark(what, ok=True):
        seen[what] = seen.get(what, False) or bool(ok)
    decisions = ("stage_packed", "stage_mform", "dev_parse", "dev_mform", "direct_out", "keep_on_device")
    for what in ["table " + t for t in TABLE_NAMES] + [d + v for d in decisions for v in (" on", " off")] + \
            ["error code", "ranges asked and cut", "ranges asked, one piece", "automatic range count", "range_unit > 1", "range_unit == 1 in ranges",
             "both parsers have work", "blocks_possible binds", "several chunks", "auto takes the device", "auto takes the host",
             "pinned below the line", "packed asked, byte planes win", "form dropped: no stream has one", "packed dropped: no stream has it", "form dropped: arena past 2^36",
             "device form dropped: too many streams", "ranges dropped: too many streams", "ranges dropped: a stream for the host",
             "ranges dropped: device-resident output", "pk_ntiles preset", "a job without the form beside ones with it"]:
        mark(what, False)
    for case, res in zip(cases, results):
        mark("error code", res["rc"] == capi.ERR_ARG)
        if res["rc"] != 0:
            continue
        t = decode(res)
        tot = t["totals"]
        asked = (case.flags >> 8) & 0xFF
        default_staging = not case.flags & (capi.BATCH_STAGE_INT16 | capi.BATCH_STAGE_PACKED) and not case.prestaged and not case.plan_flags
        for name in TABLE_NAMES:
            mark("table " + name, name in t)
        for d in decisions:
            mark(d + (" on" if tot[d] else " off"))
        mark("ranges asked and cut", asked > 1 and tot["R"] == asked)
        mark("ranges asked, one piece", asked > 1 and tot["R"] == 1)
        mark("automatic range count", asked == 0 and tot["R"] > 1)
        if "slots" in t:
            live = t["slots"][t["slots"]["ok"] == 1]
            if tot["R"] > 1:
                mark("range_unit > 1", (live["range_unit"] > 1).any())
                mark("range_unit == 1 in ranges", (live["range_unit"] == 1).any())
            promised = [-(-s[2] // (s[1] << s[0])) for s in case.streams if s[6]]
            mark("blocks_possible binds", (live["need_blocks"] < np.array(promised, dtype="u8")).any())
            mark("pk_ntiles preset", (live["pk_ntiles"] > 0).any())
            n_live = len(live)
        else:
            n_live = 0
        mark("both parsers have work", "dev_ids" in t and "host_ids" in t)
        mark("several chunks", "chunks" in t and len(t["chunks"]) > 2)
        if case.parse == capi.PARSE_AUTO and n_live:
            mark("auto takes the device" if tot["dev_parse"] else "auto takes the host")
        mark("pinned below the line", case.flags & capi.BATCH_PCM_PINNED and case.d_pcm_words is None and not tot["direct_out"] and tot["R"] == 1)
        mark("packed asked, byte planes win", case.flags & capi.BATCH_STAGE_PACKED and tot["stage_mform"])
        mark("form dropped: no stream has one", default_staging and n_live and tot["mf_total"] == 0 and not tot["stage_mform"] and not tot["dev_mform"])
        mark("packed dropped: no stream has it", case.flags & capi.BATCH_STAGE_PACKED and not case.flags & capi.BATCH_STAGE_BYTEPLANE and
             not case.plan_flags and not tot["dev_parse"] and n_live and not tot["stage_packed"])
        mark("form dropped: arena past 2^36", default_staging and tot["mf_total"] >> 36 and not tot["stage_mform"] and not tot["dev_mform"])
        nd = len(t.get("dev_ids", ()))
        mark("device form dropped: too many streams", default_staging and 0 < tot["mf_total"] < 1 << 36 and nd > RANGE_MAX_STREAMS and not tot["dev_mform"])
        if asked > 1 and asked <= 64 and tot["dev_parse"] and tot["R"] == 1 and nd:
            mark("ranges dropped: too many streams", nd > RANGE_MAX_STREAMS)
            mark("ranges dropped: a stream for the host", "host_ids" in t)
            mark("ranges dropped: device-resident output", tot["keep_on_device"])
        if "jobs" in t:
            mark("a job without the form beside ones with it", (t["jobs"]["mf_rows"] == 0).any() and (t["jobs"]["mf_rows"] > 0).any())
    return seen


# ---------------------------------------------------------------------------------------------------------------- the tests

_state = {}


def _all():
    if not _state:
        L = _lib()
        _state["L"] = L
        _state["cases"] = build_cases(L)
        _state["results"] = [run_case(L, c) for c in _state["cases"]]
    return _state["L"], _state["cases"], _state["results"]


def test_equal_to_the_recorded_front_end():
    _, cases, results = _all()
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["recorded_from"], "the fixture names the commit whose front end it was recorded from"
    got = recording(cases, results)
    # no case is left out: the fixture has one fingerprint per case of the list, and names are part of what is hashed
    assert len(got["case_sha256_16"]) == len(golden["case_sha256_16"]) == len(cases)
    wrong = [c.name for c, a, b in zip(cases, got["case_sha256_16"], golden["case_sha256_16"]) if a != b]
    assert not wrong, "%d of %d cases differ from the recorded front end, first: %r" % (len(wrong), len(cases), wrong[:3])
    assert got["errors"] == golden["errors"]
    assert got["sha256_of_all"] == golden["sha256_of_all"]


def test_case_list_covers_the_layout():
    _, cases, results = _all()
    missing = [what for what, ok in coverage(cases, results).items() if not ok]
    assert not missing, missing


def _disjoint(intervals, what):
    last = 0
    for a, b in sorted(i for i in intervals if i[1] > i[0]):
        assert a >= last, "%s: [%d, %d) overlaps what ends at %d" % (what, a, b, last)
        last = b


def _deliverable(total, block_len, channels, blocks):
    pos = 0
    for _ in range(blocks):
        if pos >= total:
            break
        take = min(block_len, total - pos)
        if channels > 1:
            take -= take % channels
        pos += take
        if take != block_len:
            break
    return pos


def test_arenas_and_chunks():
    """arena slices of live streams are disjoint and 64-word aligned; every live stream lies in exactly one chunk, and the chunks' ranges
    tile the arenas; every live stream has exactly one parser"""
    _, cases, results = _all()
    for case, res in zip(cases, results):
        if res["rc"] != 0 or not case.streams:
            continue
        t = decode(res)
        slots, chunks, tot = t["slots"], t["chunks"], t["totals"]
        live = np.flatnonzero(slots["ok"])
        assert [int(i) for i in live] == [k for k, s in enumerate(case.streams) if s[6]], case.name
        s = slots[live]
        assert not (s["idx_off"] % 64).any() and not (s["idx_len"] % 64).any() and (s["pcm_off"] == s["idx_off"]).all(), case.name
        # (arena order is stream order: adjacent slices meet exactly)
        assert (s["idx_off"][1:] == s["idx_off"][:-1] + s["idx_len"][:-1]).all() and (s["hdr_off"][1:] == s["hdr_off"][:-1] + s["need_blocks"][:-1]).all()
        if len(s):
            assert int(s["idx_off"][0]) == 0 and int(s["idx_off"][-1] + s["idx_len"][-1]) == tot["idx_total"] == tot["pcm_total"], case.name
            assert int(s["hdr_off"][-1] + s["need_blocks"][-1]) == tot["hdr_total"], case.name
        for form, off, size in (("mf", "mf_off", None), ("pk", "pk_chunk_off", "pk_chunk_cap")):
            if size:
                _disjoint([(int(x[off]), int(x[off] + x[size])) for x in s], case.name + " " + form)
        assert not (s["mf_off"] % 256).any(), case.name
        # chunks: [first, last) tile the items; a live stream's slices lie inside its chunk's ranges, which tile the arenas
        assert int(chunks["first"][0]) == 0 and int(chunks["last"][-1]) == len(case.streams), case.name
        assert (chunks["first"][1:] == chunks["last"][:-1]).all(), case.name
        for i in live:
            c = chunks[int(slots[i]["chunk"])]
            assert c["first"] <= i < c["last"] and c["idx_begin"] <= slots[i]["idx_off"] and slots[i]["idx_off"] + slots[i]["idx_len"] <= c["idx_end"]
            assert c["hdr_begin"] <= slots[i]["hdr_off"] and slots[i]["hdr_off"] + slots[i]["need_blocks"] <= c["hdr_end"], case.name
        used = chunks[chunks["idx_end"] > chunks["idx_begin"]]
        if len(used):
            assert int(used["idx_begin"][0]) == 0 and int(used["idx_end"][-1]) == tot["idx_total"], case.name
            assert (used["idx_begin"][1:] == used["idx_end"][:-1]).all() and (used["hdr_begin"][1:] == used["hdr_end"][:-1]).all(), case.name
        for a, b, total in (("mf_begin", "mf_end", "mf_total"), ("mf_pair_begin", "mf_pair_end", "mf_pairs_total"), ("pk_chunk_begin", "pk_chunk_end", "pk_chunks_total")):
            if tot[total]:
                assert int(chunks[a][0]) == 0 and int(chunks[b][-1]) == tot[total] and (chunks[a][1:] == chunks[b][:-1]).all(), (case.name, total)
        # parsers
        dev, host = [int(x) for x in t.get("dev_ids", ())], [int(x) for x in t.get("host_ids", ())]
        assert sorted(dev + host) == [int(i) for i in live] and not set(dev) & set(host), case.name
        assert [int(i) for i in np.flatnonzero(slots["on_dev"])] == dev, case.name
        want_out = [k for k, st in enumerate(case.streams) if st[6] and st[7]] if not tot["keep_on_device"] and not tot["direct_out"] else []
        assert [int(x) for x in t.get("out_ids", ())] == want_out, case.name


def test_block_ranges_and_stripes():
    """piece_len over the ranges sums to what every stream delivers; the pieces of one range are disjoint and lie inside the range's part
    of the PCM arena; the stripes tile the file arena"""
    _, cases, results = _all()
    checked = 0
    for case, res in zip(cases, results):
        if res["rc"] != 0 or not case.streams:
            continue
        t = decode(res)
        tot, n = t["totals"], len(case.streams)
        R = tot["R"]
        if R == 1:
            assert "piece_len" not in t and "stripe_at" not in t and tot["pcm_arena_words"] == tot["pcm_total"], case.name
            continue
        plen, poff, rbase = t["piece_len"].reshape(R, n), t["piece_off"].reshape(R, n), t["rbase"]
        assert len(rbase) == R + 1 and int(rbase[0]) == 0 and tot["pcm_arena_words"] >= int(rbase[R]) and not tot["direct_out"], case.name
        for i, st in enumerate(case.streams):
            if not st[6]:
                assert not plen[:, i].any()
                continue
            blocks = int(t["slots"][i]["need_blocks"])
            assert int(plen[:, i].sum()) == _deliverable(st[2], st[1] << st[0], st[3], blocks), (case.name, i)
        for r in range(R):
            live = [i for i in range(n) if case.streams[i][6]]
            _disjoint([(int(poff[r, i]), int(poff[r, i] + plen[r, i])) for i in live], "%s range %d" % (case.name, r))
            for i in live:
                assert rbase[r] <= poff[r, i] and poff[r, i] + plen[r, i] <= rbase[r + 1] and poff[r, i] % 64 == 0, (case.name, r, i)
        nd = len(t["dev_ids"])
        at, base = t["stripe_at"].reshape(R, nd), t["stripe_base"]
        flat = at.reshape(-1)
        assert int(flat[0]) == 0 and (flat[1:] >= flat[:-1]).all() and int(base[R]) == tot["files_total"], case.name
        assert [int(x) for x in base[:R]] == [int(x) for x in at[:, 0]], case.name
        # every file's slot is covered: the stripes of stream k add up to its slot
        ends = np.append(flat[1:], base[R])
        per_stream = (ends - flat).reshape(R, nd).sum(axis=0)
        slot = [(case.streams[int(i)][5] + 15) // 16 * 16 + 16 for i in t["dev_ids"]]
        assert [int(x) for x in per_stream] == slot, case.name
        checked += 1
    assert checked > 100


def test_jobs():
    """every job's byte-plane rows are whole tiles of its level's lean kernel and fit the stream's reservation; file slots are disjoint"""
    L, cases, results = _all()
    checked = 0
    for case, res in zip(cases, results):
        if res["rc"] != 0:
            continue
        t = decode(res)
        if "jobs" not in t:
            continue
        jobs, slots, tot = t["jobs"], t["slots"], t["totals"]
        assert len(jobs) == len(t["dev_ids"]) and tot["jobs_bytes"] >= 72 * len(jobs) and tot["res_bytes"] == 20 * len(jobs), case.name
        _disjoint([(int(j["file_off"]), int(j["file_off"]) + (int(j["file_len"]) + 15) // 16 * 16 + 16) for j in jobs], case.name)
        cols = 0
        for j, i in zip(jobs, t["dev_ids"]):
            s = slots[int(i)]
            assert j["idx_off"] == s["idx_off"] and j["hdr_off"] == s["hdr_off"] and j["blocks"] == s["need_blocks"] and j["col_off"] == cols
            cols += int(j["blocks"]) << int(j["level"])
            if j["mf_rows"]:
                tile = L.acmk_tile2_rows(int(j["level"]))
                assert tot["dev_mform"] and tile and j["mf_rows"] % tile == 0 and j["mf_rows"] <= s["mf_rows_cap"], (case.name, int(i))
                assert j["mf_off"] == s["mf_off"] and j["mf_pair_off"] == s["mf_pair_off"], case.name
                assert s["pk_ntiles"] * L.acmk_tile2m_rows(int(j["level"])) == j["mf_rows"], case.name
            else:
                assert s["pk_ntiles"] == 0, case.name
        assert cols == tot["cols_total"], case.name
        groups = t["groups"]
        used = groups[groups["k_last"] > groups["k_first"]]
        assert int(used["k_first"][0]) == 0 and int(used["k_last"][-1]) == len(jobs) and (used["k_first"][1:] == used["k_last"][:-1]).all(), case.name
        assert int(used["file_begin"][0]) == 0 and int(used["file_end"][-1]) == tot["files_total"], case.name
        checked += 1
    assert checked > 100
