"""The windowed batch decode's device-free half (libacm_amd/csrc/acm_window_layout.cpp), without a GPU.

acmk_window_layout_visit() computes from probed headers, file lengths, block indices, the windows and the options alone which blocks
every window stages, where its rows, headers, columns, file span and PCM slot sit, which windows the device parser takes, the job
records it reads and the sizes of the job arena.  Three kinds of check over one list of cases:

  * an exact model: a pure-Python restatement of the rules (words / status / block range from tests/test_block_index.py::expected_window)
    that every table must equal;
  * properties of the tables themselves: slots in window order, disjoint and whole multiples of 64 words, arena regions that are
    disjoint prefix sums, file slots with their slack, block walks inside their spans, every active window with exactly one parser;
  * equality with the front end before the split: the SHA-256 of every table equals what acm_batch_decode_windows of the commit named in
    tests/golden/window_layout.json computed for the same case (recorded from that commit's own lines by
    tests/golden/make_golden_window_layout.py through the dry-run seam in profiles/window_layout_parent_seam.patch).

Items are numbers and synthetic mark arrays; no file image is read, so a span of 256 MiB costs nothing.
"""
import ctypes as C
import hashlib
import json
import os
from types import SimpleNamespace

import numpy as np

from libacm_amd import capi
from test_block_index import expected_window
from test_gpu_windows import window_kinds

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_layout.json")

SLOT_FIELDS = ("status", "words", "slot_off", "slot_words", "dev_off", "active", "on_device", "b0", "nb", "row_begin", "lead", "idx_off",
               "hdr_off", "col_off", "span_lo", "span_len", "file_off")
SLOT = np.dtype([(f, "<i8" if f == "status" else "<u8") for f in SLOT_FIELDS])
JOB = np.dtype([("file_off", "<u8"), ("idx_off", "<u8"), ("hdr_off", "<u8"), ("col_off", "<u8"), ("file_len", "<u4"), ("data_start", "<u4"),
                ("level", "<u4"), ("rows", "<u4"), ("blocks", "<u4"), ("range_unit", "<u4"), ("mf_off", "<u8"), ("mf_pair_off", "<u4"),
                ("mf_rows", "<u4")])
BJOB = np.dtype([(f, "<u4") for f in ("job", "block", "bit", "end_bit", "h20", "pad")])
TOTALS = ("idx_total", "hdr_total", "pcm_total", "cols_total", "files_total", "max_columns", "blocks_parsed", "jobs_bytes", "bjobs_bytes",
          "res_bytes", "dev_parse", "rc")
DTYPES = {"slots": SLOT, "act": "<u8", "dev_ids": "<u8", "host_ids": "<u8", "jobs": JOB, "bjobs": BJOB, "totals": "<i8"}
AUTO_BLOCKS = 256               # ACM_WINDOWS_AUTO_BLOCKS
SPAN_LIMIT = 1 << 28            # acmk_parse_supported: spans below 256 MiB
RESULT_BYTES = 16 + 4           # sizeof(AcmParseResult) + its flag word

VISIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_size_t)


def _lib():
    L = capi.lib()
    L.acmk_window_layout_visit.argtypes = [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, VISIT, C.c_void_p]
    return L


def round_up(v, a):
    return (v + a - 1) // a * a


# ---------------------------------------------------------------------------------------------------------------- items and cases

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


def item(level, rows, blocks, short_by=0, channels=1, header_bytes=14, end_status=0, bits=None, length=None):
    """what the driver's first step makes of a whole, plausibly indexed file of `blocks` blocks - and a mark array to go with it.  bits[b]:
    the length of block b (default: its header, a code per column, about six bits a sample)"""
    cols, bl = 1 << level, rows << level
    total = max(blocks * bl - short_by, 1)
    at, bit = 8 * header_bytes, []
    for b in range(blocks):
        bit.append(at)
        at += bits[b] if bits else 20 + 5 * cols + 6 * bl + b * 7 % 13
    bit.append(at)
    marks = np.zeros(blocks + 1, dtype=capi.BLOCK_MARK_DT)
    marks["bit"] = bit
    marks["val"][:blocks] = [(b * 40503 + 7 * level + rows) & 0xFFFF for b in range(blocks)]
    marks["pwr"][:blocks] = [(b + level) % 16 for b in range(blocks)]
    whole = _deliverable(total, bl, channels, blocks)
    info = SimpleNamespace(level=level, rows=rows, cols=cols, channels=channels, total_values=total, header_bytes=header_bytes,
                           blocks=blocks, end_status=end_status)
    return SimpleNamespace(info=info, len=(at + 7) // 8 if length is None else length, ok=1, end_status=end_status, whole=whole, marks=marks,
                           st=SimpleNamespace(words=whole, block_len=bl, info=info))


def not_ok(end_status):
    """a file that is not ACM (its probe's code), or one whose index was refused (ACMHIP_ERR_ARG): nothing to deliver, no marks to read"""
    info = SimpleNamespace(level=0, rows=0, cols=0, channels=0, total_values=0, header_bytes=0, blocks=0, end_status=0)
    return SimpleNamespace(info=info, len=200, ok=0, end_status=end_status, whole=0, marks=None, st=None)


class Case:
    def __init__(self, name, items, wins, parse=capi.PARSE_HOST, d_pcm_words=None):
        self.name, self.items, self.wins, self.parse, self.d_pcm_words = name, items, wins, parse, d_pcm_words


PARSES = {"host": capi.PARSE_HOST, "device": capi.PARSE_DEVICE, "auto": capi.PARSE_AUTO}


def matrix_items(level):
    """tests/test_gpu_windows.py::matrix_stream as numbers: 3 to 40 blocks, a ragged end, mono and stereo"""
    out = []
    for rows in (1, 3, 16, 255):
        bl = rows << level
        nb = 3 if bl >= 4096 else min(40, 4096 // bl + 3)
        out.append(item(level, rows, nb, short_by=max(1, bl // 3) if bl > 1 else 0, channels=1 + ((level + rows) % 2 if bl % 2 == 0 else 0)))
    return out


def build_cases():
    cases = [Case("empty", [], []), Case("no_windows", [item(5, 4, 6)], [], parse=capi.PARSE_DEVICE)]
    for level in (0, 5, 9, 15):
        items = matrix_items(level)
        wins = [(f, a, n) for f, it in enumerate(items) for a, n in window_kinds(it)]
        for parse in PARSES:
            cases.append(Case("kinds_l%d_%s" % (level, parse), items, wins, parse=PARSES[parse]))
    # items nobody can decode among ones that are fine: an item that does not exist, a foreign file, a refused index
    odd = [item(7, 16, 12), not_ok(-3), not_ok(capi.ERR_ARG), item(5, 3, 9, short_by=11, end_status=-6)]
    wins = [(0, 100, 5000), (4, 0, 10), (1, 0, 100), (1, 5, 0), (2, 7, 64), (3, 50, 400), (3, 800, 5000), (77, 0, 1), (0, 20000, 9000)]
    for parse in PARSES:
        cases.append(Case("undecodable_" + parse, odd, wins, parse=PARSES[parse]))
    # ACM_BATCH_PARSE_AUTO on both sides of its threshold, in one window and spread over many
    long = item(5, 4, 300)
    bl = long.st.block_len
    for blocks in (AUTO_BLOCKS - 1, AUTO_BLOCKS):
        cases.append(Case("auto_%d_one" % blocks, [long], [(0, 0, blocks * bl)], parse=capi.PARSE_AUTO))
        cases.append(Case("auto_%d_many" % blocks, [long, long], [(k % 2, 2 * bl * k + bl // 2, bl) for k in range(blocks // 2)] +
                          [(1, 0, bl)] * (blocks % 2), parse=capi.PARSE_AUTO))
    # one call with windows for both parsers: a block of 2^28 bytes, and an index whose last mark lies in the reader's virtual zero byte
    fat = item(5, 4, 3, bits=[4000, 8 * SPAN_LIMIT, 4000])
    tail = item(5, 4, 6)
    tail.len = int(tail.marks["bit"][6]) // 8 + 1
    tail.marks["bit"][6] = 8 * tail.len + 1
    bl = fat.st.block_len
    mixed = [(0, 0, 100), (0, bl + 5, 64), (1, 0, 200), (1, 5 * bl + 7, 100), (0, 2 * bl + 3, 40), (1, 0, 6 * bl)]
    for parse in ("device", "host"):
        cases.append(Case("mixed_" + parse, [fat, tail], mixed, parse=PARSES[parse]))
    # device-resident output: exactly enough room, one word short
    items = matrix_items(7)
    wins = [(f, a, n) for f, it in enumerate(items) for a, n in window_kinds(it)]
    need = model(Case("", items, wins))["totals"]["pcm_total"]
    for parse in ("host", "device"):
        cases.append(Case("d_pcm_exact_" + parse, items, wins, parse=PARSES[parse], d_pcm_words=need))
        cases.append(Case("d_pcm_short_" + parse, items, wins, parse=PARSES[parse], d_pcm_words=need - 1))
    return cases


# ---------------------------------------------------------------------------------------------------------------- the model

def model(case):
    """every table as the rules of acm_window_layout.h give it: {"slots": [dict], "act", "dev_ids", "host_ids": [int], "jobs", "bjobs":
    [tuple], "totals": dict}"""
    items, n = case.items, len(case.items)
    slots, act = [], []
    t = dict.fromkeys(TOTALS, 0)
    for f, first, count in case.wins:
        s = dict.fromkeys(SLOT_FIELDS, 0)
        s["slot_off"] = s["dev_off"] = t["pcm_total"]
        slots.append(s)
        if f >= n:
            s["status"] = capi.ERR_ARG
            continue
        it = items[f]
        words, s["status"], b0, nb = expected_window(it.st, it.end_status, first, count)
        if not words:
            continue
        cols, rows = it.info.cols, it.info.rows
        first_row = first // cols
        lead = first - first_row * cols
        s.update(words=words, active=1, b0=b0, nb=nb, row_begin=first_row - b0 * rows, lead=lead, idx_off=t["idx_total"], hdr_off=t["hdr_total"],
                 slot_words=round_up(lead + words, 64), dev_off=s["slot_off"] + lead)
        t["idx_total"] += round_up(nb * rows * cols, 64)
        t["hdr_total"] += nb
        t["pcm_total"] += s["slot_words"]
        t["blocks_parsed"] += nb
        act.append(len(slots) - 1)
    t["dev_parse"] = int(case.parse == capi.PARSE_DEVICE or (case.parse == capi.PARSE_AUTO and t["blocks_parsed"] >= AUTO_BLOCKS))
    dev_ids, host_ids = [], []
    for k in act:
        s, it = slots[k], items[case.wins[k][0]]
        if t["dev_parse"]:
            lo, hi = int(it.marks["bit"][s["b0"]]), int(it.marks["bit"][s["b0"] + s["nb"]])
            s["span_lo"] = lo // 8 & ~3
            s["span_len"] = min(it.len, (hi + 7) // 8) - s["span_lo"]
            supported = it.info.rows >= 1 and s["nb"] >= 1 and s["span_len"] < SPAN_LIMIT and s["nb"] << it.info.level < 0xFFFFFFFF
            s["on_device"] = int(supported and hi - 8 * s["span_lo"] <= 8 * s["span_len"])
        if not s["on_device"]:
            host_ids.append(k)
            continue
        s["file_off"], s["col_off"] = t["files_total"], t["cols_total"]
        t["files_total"] += round_up(s["span_len"], 16) + 16
        t["cols_total"] += s["nb"] * it.info.cols
        t["max_columns"] = max(t["max_columns"], s["nb"] * it.info.cols)
        dev_ids.append(k)
    out = {"slots": slots, "act": act, "dev_ids": dev_ids, "host_ids": host_ids, "jobs": [], "bjobs": [], "totals": t}
    if (case.d_pcm_words is not None and case.d_pcm_words < t["pcm_total"]) or len(dev_ids) > 0xFFFFFFFF or t["hdr_total"] > 0xFFFFFFFF:
        t["rc"] = capi.ERR_ARG
        return out
    for a, k in enumerate(dev_ids):
        s, it = slots[k], items[case.wins[k][0]]
        out["jobs"].append((s["file_off"], s["idx_off"], s["hdr_off"], s["col_off"], s["span_len"], 0, it.info.level, it.info.rows, s["nb"], 1, 0, 0, 0))
        for b in range(s["nb"]):
            m, nxt = it.marks[s["b0"] + b], it.marks[s["b0"] + b + 1]
            out["bjobs"].append((a, b, int(m["bit"]) - 8 * s["span_lo"], int(nxt["bit"]) - 8 * s["span_lo"], int(m["val"]) << 4 | int(m["pwr"]), 0))
    t["jobs_bytes"] = round_up(72 * len(dev_ids), 64)
    t["bjobs_bytes"] = round_up(24 * len(out["bjobs"]), 64)
    t["res_bytes"] = RESULT_BYTES * len(dev_ids)
    return out


# ---------------------------------------------------------------------------------------------------------------- running, recording

def run_case(L, case):
    """{"rc", "tables": {name: bytes}, "elem": {name: elem_bytes}} in visiting order"""
    n, nwin = len(case.items), len(case.wins)
    info = (capi.StageInfo * max(n, 1))()
    length, whole = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
    ok, end_status, blocks = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint32)
    marks = (C.c_void_p * max(n, 1))()
    for i, it in enumerate(case.items):
        f = it.info
        info[i] = capi.StageInfo(f.level, f.rows, f.cols, f.channels, f.channels, 22050, f.total_values, 0, f.blocks, f.end_status, 0, f.header_bytes)
        length[i], whole[i], ok[i], end_status[i], blocks[i] = it.len, it.whole, it.ok, it.end_status, f.blocks
        marks[i] = it.marks.ctypes.data if it.marks is not None else None
    win3 = np.array(case.wins, dtype=np.uint64).reshape(-1)
    opts = capi.BatchOpts(0, 0, 4, 0, case.parse, 0, 0x100 if case.d_pcm_words is not None else None, case.d_pcm_words or 0, None)
    tables, elem = {}, {}

    def visit(_ctx, name, data, elem_bytes, count):
        name = name.decode()
        assert name not in tables
        tables[name] = C.string_at(data, elem_bytes * count)
        elem[name] = elem_bytes
    rc = L.acmk_window_layout_visit(info, length.ctypes.data, ok.ctypes.data, end_status.ctypes.data, whole.ctypes.data, marks, blocks.ctypes.data,
                                    n, win3.ctypes.data if nwin else None, nwin, C.byref(opts), VISIT(visit), None)
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
            "errors": {c.name: r["rc"] for c, r in zip(cases, results) if r["rc"] != 0}, "case_sha256_16": {c.name: e[:16] for c, e in zip(cases, each)}}


def decode(res):
    """the visited tables in the model's shape"""
    t = {}
    for name, dt in DTYPES.items():
        raw = res["tables"].get(name, b"")
        if name in res["elem"]:
            assert np.dtype(dt).itemsize == res["elem"][name], name
        t[name] = np.frombuffer(raw, dtype=dt)
    out = {"slots": [dict(zip(SLOT_FIELDS, r)) for r in t["slots"].tolist()], "jobs": t["jobs"].tolist(), "bjobs": t["bjobs"].tolist()}
    out.update({name: t[name].tolist() for name in ("act", "dev_ids", "host_ids")})
    assert len(t["totals"]) == len(TOTALS)
    out["totals"] = dict(zip(TOTALS, t["totals"].tolist()))
    return out


_state = {}


def _all():
    if not _state:
        L = _lib()
        _state["cases"] = build_cases()
        _state["results"] = [run_case(L, c) for c in _state["cases"]]
    return _state["cases"], _state["results"]


def coverage(cases, results):
    """what the case list reaches, as {condition: bool}; every one must hold"""
    seen = dict.fromkeys(("error code", "both parsers have work", "auto takes the host", "auto takes the device", "a span too long for the device",
                          "a last mark behind the span", "an inactive window", "a window of an item that does not exist", "a lead", "a halo block"), False)
    for case, res in zip(cases, results):
        t = decode(res)
        tot = t["totals"]
        seen["error code"] |= res["rc"] == capi.ERR_ARG
        seen["both parsers have work"] |= bool(tot["dev_parse"] and t["dev_ids"] and t["host_ids"])
        if case.parse == capi.PARSE_AUTO and t["act"]:
            seen["auto takes the device" if tot["dev_parse"] else "auto takes the host"] = True
        for k in t["host_ids"] if tot["dev_parse"] else ():
            s = t["slots"][k]
            hi = int(case.items[case.wins[k][0]].marks["bit"][s["b0"] + s["nb"]])
            seen["a span too long for the device"] |= s["span_len"] >= SPAN_LIMIT
            seen["a last mark behind the span"] |= s["span_len"] < SPAN_LIMIT and hi > 8 * (s["span_lo"] + s["span_len"])
        seen["an inactive window"] |= any(not s["active"] for s in t["slots"])
        seen["a window of an item that does not exist"] |= any(w[0] >= len(case.items) for w in case.wins)
        seen["a lead"] |= any(s["lead"] for s in t["slots"])
        seen["a halo block"] |= any(s["active"] and s["row_begin"] >= case.items[w[0]].info.rows for s, w in zip(t["slots"], case.wins))
    return seen


# ---------------------------------------------------------------------------------------------------------------- the tests

def test_equal_to_the_model():
    cases, results = _all()
    for case, res in zip(cases, results):
        got, want = decode(res), model(case)
        assert res["rc"] == want["totals"]["rc"], case.name
        for name in ("totals", "act", "dev_ids", "host_ids", "jobs", "bjobs"):
            assert got[name] == want[name], (case.name, name)
        assert len(got["slots"]) == len(want["slots"]), case.name
        for k, (a, b) in enumerate(zip(got["slots"], want["slots"])):
            assert a == b, (case.name, k, case.wins[k])


def test_case_list_covers_the_layout():
    cases, results = _all()
    missing = [what for what, ok in coverage(cases, results).items() if not ok]
    assert not missing, missing


def test_properties():
    """what must hold for any call: slots in window order, disjoint, whole multiples of 64 words, the first wanted sample `lead` words
    in; the idx / hdr / col / file regions disjoint prefix sums; 16-byte aligned file slots with 16 bytes of slack; every block walk inside
    its job's span; every active window with exactly one parser"""
    cases, results = _all()
    for case, res in zip(cases, results):
        t = decode(res)
        slots, tot = t["slots"], t["totals"]
        assert len(slots) == len(case.wins), case.name
        end = idx = hdr = 0
        for k, (s, (f, first, count)) in enumerate(zip(slots, case.wins)):
            assert s["slot_off"] == end and s["slot_words"] % 64 == 0, (case.name, k)
            end += s["slot_words"]
            assert bool(s["active"]) == (s["words"] > 0) == (s["slot_words"] > 0), (case.name, k)
            if not s["active"]:
                assert s["dev_off"] == s["slot_off"] and not s["on_device"], (case.name, k)
                continue
            info = case.items[f].info
            assert s["dev_off"] - s["slot_off"] == first % info.cols == s["lead"], (case.name, k)
            assert s["dev_off"] + s["words"] <= s["slot_off"] + s["slot_words"], (case.name, k)
            assert (s["idx_off"], s["hdr_off"]) == (idx, hdr) and idx % 64 == 0, (case.name, k)
            idx += round_up(s["nb"] * info.rows * info.cols, 64)
            hdr += s["nb"]
            assert s["b0"] + s["nb"] <= info.blocks and s["row_begin"] < s["nb"] * info.rows, (case.name, k)
        assert (end, idx, hdr) == (tot["pcm_total"], tot["idx_total"], tot["hdr_total"]), case.name
        assert tot["blocks_parsed"] == hdr, case.name
        assert t["act"] == [k for k, s in enumerate(slots) if s["active"]], case.name
        assert sorted(t["dev_ids"] + t["host_ids"]) == t["act"] and t["host_ids"] == sorted(t["host_ids"]), case.name
        assert t["dev_ids"] == [k for k, s in enumerate(slots) if s["on_device"]], case.name
        assert tot["dev_parse"] or not t["dev_ids"], case.name
        if res["rc"] != 0:
            assert not t["jobs"] and not t["bjobs"], case.name
            continue
        assert len(t["jobs"]) == len(t["dev_ids"]), case.name
        jobs = [dict(zip(JOB.names, j)) for j in t["jobs"]]
        file_at = col_at = nbj = 0
        for j, k in zip(jobs, t["dev_ids"]):
            s, info = slots[k], case.items[case.wins[k][0]].info
            assert j["file_off"] == s["file_off"] == file_at and file_at % 16 == 0, (case.name, k)
            file_at += round_up(j["file_len"], 16) + 16
            assert file_at - j["file_off"] >= j["file_len"] + 16, (case.name, k)
            assert j["col_off"] == s["col_off"] == col_at, (case.name, k)
            col_at += s["nb"] * info.cols
            assert (j["idx_off"], j["hdr_off"], j["file_len"], j["level"], j["rows"], j["blocks"], j["range_unit"]) == \
                (s["idx_off"], s["hdr_off"], s["span_len"], info.level, info.rows, s["nb"], 1), (case.name, k)
            assert s["span_lo"] % 4 == 0 and s["span_lo"] + s["span_len"] <= case.items[case.wins[k][0]].len, (case.name, k)
            nbj += s["nb"]
        assert (file_at, col_at) == (tot["files_total"], tot["cols_total"]), case.name
        assert tot["max_columns"] == max([slots[k]["nb"] * case.items[case.wins[k][0]].info.cols for k in t["dev_ids"]], default=0), case.name
        assert len(t["bjobs"]) == nbj, case.name
        at = 0
        for a, j in enumerate(jobs):
            for b in range(j["blocks"]):
                job, block, bit, end_bit, h20, pad = t["bjobs"][at]
                assert (job, block, pad) == (a, b, 0) and bit + 20 <= end_bit <= 8 * j["file_len"], (case.name, a, b)
                at += 1
        assert tot["jobs_bytes"] % 64 == 0 and tot["jobs_bytes"] >= 72 * len(jobs), case.name
        assert tot["bjobs_bytes"] % 64 == 0 and tot["bjobs_bytes"] >= 24 * nbj and tot["res_bytes"] == RESULT_BYTES * len(jobs), case.name


def test_auto_threshold():
    cases, results = _all()
    by_name = {c.name: decode(r)["totals"] for c, r in zip(cases, results)}
    for shape in ("one", "many"):
        below, at = by_name["auto_%d_%s" % (AUTO_BLOCKS - 1, shape)], by_name["auto_%d_%s" % (AUTO_BLOCKS, shape)]
        assert (below["blocks_parsed"], below["dev_parse"]) == (AUTO_BLOCKS - 1, 0) and (at["blocks_parsed"], at["dev_parse"]) == (AUTO_BLOCKS, 1)


def test_mixed_call():
    """one call whose windows go both ways: a block of 2^28 bytes and a last mark at 8 * len + 1 stay with the host, their neighbours
    go to the device"""
    cases, results = _all()
    t = decode(results[[c.name for c in cases].index("mixed_device")])
    assert t["dev_ids"] == [0, 2] and t["host_ids"] == [1, 3, 4, 5]
    assert t["slots"][1]["span_len"] >= SPAN_LIMIT and t["slots"][4]["span_len"] >= SPAN_LIMIT          # block 1, and block 2 behind its halo
    assert t["totals"]["blocks_parsed"] == 1 + 2 + 2 + 2 + 2 + 6
    t = decode(results[[c.name for c in cases].index("mixed_host")])
    assert not t["dev_ids"] and t["host_ids"] == [0, 1, 2, 3, 4, 5] and not t["totals"]["files_total"]


def test_refusals_and_the_empty_call():
    cases, results = _all()
    by_name = {c.name: (r["rc"], decode(r)) for c, r in zip(cases, results)}
    for parse in ("host", "device"):
        rc, t = by_name["d_pcm_exact_" + parse]
        assert rc == 0
        rc, short = by_name["d_pcm_short_" + parse]
        assert rc == capi.ERR_ARG and short["slots"] == t["slots"]              # a refused call has told its windows their slots
    rc, t = by_name["empty"]
    assert rc == 0 and not t["slots"] and not t["act"] and not any(t["totals"].values())
    rc, t = by_name["undecodable_device"]
    # (a window that asks for nothing has all it asked for, whatever its file is)
    assert [s["status"] for s in t["slots"]] == [0, capi.ERR_ARG, -3, 0, capi.ERR_ARG, 0, -6, capi.ERR_ARG, 0]
    assert [s["words"] for s in t["slots"]] == [5000, 0, 0, 0, 0, 400, 53, 0, 4576]


def test_equal_to_the_recorded_front_end():
    cases, results = _all()
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["recorded_from"], "the fixture names the commit whose front end it was recorded from"
    got = recording(cases, results)
    # no case is left out: the fixture has one fingerprint per case of the list, and names are part of what is hashed
    assert list(got["case_sha256_16"]) == list(golden["case_sha256_16"]) == [c.name for c in cases]
    wrong = [name for name, fp in got["case_sha256_16"].items() if golden["case_sha256_16"][name] != fp]
    assert not wrong, "%d of %d cases differ from the recorded front end, first: %r" % (len(wrong), len(cases), wrong[:3])
    assert got["errors"] == golden["errors"]
    assert got["sha256_of_all"] == golden["sha256_of_all"]
