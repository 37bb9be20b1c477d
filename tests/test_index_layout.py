"""The batch index build's device-free half (libacm_amd/csrc/acm_index_layout.cpp), without a GPU.

acmk_index_layout_visit() computes from probed headers, file lengths and the room for marks alone which items the device walks, how
many blocks each is asked for, where its file image and its marks sit in its group's halves of the arenas, and how the batch is cut
into groups.  Nothing is allocated beyond the tables and no file image is read, so a 256 MiB "file" is a number here.
"""
import ctypes as C

import numpy as np

from libacm_amd import capi

SLOT = np.dtype([(f, "<u8") for f in ("want_blocks", "file_off", "mark_off", "group", "on_dev")])
GROUP = np.dtype([(f, "<u8") for f in ("k_first", "k_last", "file_bytes", "marks")])
JOB = np.dtype([("file_off", "<u8"), ("idx_off", "<u8"), ("hdr_off", "<u8"), ("col_off", "<u8"), ("file_len", "<u4"), ("data_start", "<u4"),
                ("level", "<u4"), ("rows", "<u4"), ("blocks", "<u4"), ("range_unit", "<u4"), ("mf_off", "<u8"), ("mf_pair_off", "<u4"),
                ("mf_rows", "<u4")])
DTYPES = {"slots": SLOT, "groups": GROUP, "jobs": JOB, "dev_ids": "<u8", "host_ids": "<u8", "totals": "<u8"}
MARK = 16                       # sizeof(acm_block_mark)
RANGE_MAX_STREAMS = 32768       # ACM_PARSE_RANGE_MAX_STREAMS
DEFAULT_BUDGET = 1 << 30

VISIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_size_t)


def stream(level, rows, blocks, bits_per_sample=6, header_bytes=14, length=None, max_blocks=None, ok=1, has_marks=1, short_by=0):
    """(level, rows, total_values, header_bytes, len, max_blocks, ok, has_marks) of a stream of `blocks` blocks in a file of a plausible length"""
    bl = rows << level
    total = max(blocks * bl - short_by, 1)
    if length is None:
        length = header_bytes + (blocks * (20 + (5 << level) + bl * bits_per_sample) + 7) // 8
    return (level, rows, total, header_bytes, length, blocks if max_blocks is None else max_blocks, ok, has_marks)


def layout(streams, budget=0):
    L = capi.lib()
    L.acmk_index_layout_visit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, VISIT, C.c_void_p]
    n = len(streams)
    info = (capi.StageInfo * max(n, 1))()
    lens, room = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
    ok, has = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
    for i, (level, rows, total, hb, length, mb, o, h) in enumerate(streams):
        info[i].level, info[i].rows, info[i].cols, info[i].total_values, info[i].header_bytes = level, rows, 1 << level, total, hb
        info[i].channels = info[i].hdr_channels = 1
        lens[i], room[i], ok[i], has[i] = length, mb, o, h
    tables = {}

    def visit(ctx, name, data, elem, count):
        dt = np.dtype(DTYPES[name.decode()])
        assert dt.itemsize == elem, (name, dt.itemsize, elem)
        tables[name.decode()] = np.frombuffer(C.string_at(data, elem * count), dtype=dt).copy()
    rc = L.acmk_index_layout_visit(info, lens.ctypes.data, room.ctypes.data, ok.ctypes.data, has.ctypes.data, n, budget, VISIT(visit), None)
    assert rc == 0
    for t, dt in DTYPES.items():
        tables.setdefault(t, np.zeros(0, dtype=dt))
    return tables


def promised(s):
    level, rows, total = s[0], s[1], s[2]
    bl = rows << level
    return (total + bl - 1) // bl


def check_properties(streams, T, budget):
    """what must hold for any batch: who is on the device, 16-byte aligned slots with 16 bytes of slack, disjoint mark regions, jobs that say
    what the slots say, groups inside the budget and the stream count"""
    n = len(streams)
    budget = budget or DEFAULT_BUDGET
    # (plain Python values: a batch of 32 K streams is checked item by item)
    slots = [dict(zip(SLOT.names, r)) for r in T["slots"].tolist()]
    groups = [dict(zip(GROUP.names, r)) for r in T["groups"].tolist()]
    jobs = [dict(zip(JOB.names, r)) for r in T["jobs"].tolist()]
    dev_ids, host_ids = T["dev_ids"].tolist(), T["host_ids"].tolist()
    assert len(slots) == n and sorted(dev_ids + host_ids) == list(range(n))
    assert len(jobs) == len(dev_ids)
    on_device = set(dev_ids)
    supported = capi.lib().acmk_parse_supported
    supported.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]
    for i, s in enumerate(streams):
        level, rows, total, hb, length, mb, ok, has = s
        want = min(promised(s), mb) if ok else 0
        assert slots[i]["want_blocks"] == want
        # a header that promises more blocks than the bytes can hold stays off the device, unless fewer are asked for than even these bytes hold
        possible = (max(0, length - hb) * 8 + 8) // (20 + (5 << level)) + 1
        holds = bool(ok) and (promised(s) <= possible or want < possible)
        on_dev = bool(ok and has and want >= 1 and holds and supported(level, rows, length, want))
        assert bool(slots[i]["on_dev"]) == on_dev, (i, s)
        assert (i in on_device) == on_dev
    assert T["totals"][3] == T["slots"]["want_blocks"].sum()
    covered = 0
    for g, gr in enumerate(groups):
        k0, k1 = int(gr["k_first"]), int(gr["k_last"])
        assert k0 == covered and k1 > k0
        covered = k1
        assert k1 - k0 <= RANGE_MAX_STREAMS
        file_at = mark_at = 0
        for k in range(k0, k1):
            i = int(dev_ids[k])
            s, sl, j = streams[i], slots[i], jobs[k]
            assert sl["group"] == g
            # the slot: 16-byte aligned, behind the one in front of it, the file and >= 16 (zero) bytes of slack inside it
            assert sl["file_off"] % 16 == 0 and sl["file_off"] == file_at
            file_at += (s[4] + 15) // 16 * 16 + 16
            assert file_at - sl["file_off"] >= s[4] + 16
            # the marks: want + 1 entries nobody else has
            assert sl["mark_off"] == mark_at
            mark_at += int(sl["want_blocks"]) + 1
            assert (j["file_off"], j["hdr_off"], j["file_len"], j["data_start"], j["level"], j["rows"], j["blocks"]) == \
                (sl["file_off"], sl["mark_off"], s[4], s[3], s[0], s[1], sl["want_blocks"])
            assert (j["idx_off"], j["col_off"], j["range_unit"], j["mf_off"], j["mf_pair_off"], j["mf_rows"]) == (0, 0, 0, 0, 0, 0)
        assert (gr["file_bytes"], gr["marks"]) == (file_at, mark_at)
        cost = file_at + MARK * mark_at
        assert cost <= budget or k1 - k0 == 1, (g, cost, budget)
        # (greedy: the next stream would not have fitted)
        if g + 1 < len(groups):
            nxt = streams[int(dev_ids[k1])]
            nxt_cost = (nxt[4] + 15) // 16 * 16 + 16 + MARK * (int(slots[int(dev_ids[k1])]["want_blocks"]) + 1)
            assert cost + nxt_cost > budget or k1 - k0 == RANGE_MAX_STREAMS
    assert covered == len(dev_ids)
    if len(groups):
        assert T["totals"][0] == T["groups"]["file_bytes"].max() and T["totals"][1] == T["groups"]["marks"].max()
        assert T["totals"][2] == (T["groups"]["k_last"] - T["groups"]["k_first"]).max()
    else:
        assert tuple(T["totals"][:3]) == (0, 0, 0)


def mixed():
    out = []
    for i in range(60):
        lv, rows, nb = [7, 9, 5, 3, 11, 0, 13, 8][i % 8], [16, 3, 1, 33][i % 4], 1 + (i * 7) % 23
        out.append(stream(lv, rows, nb, header_bytes=42 if i % 9 == 4 else 14, short_by=(i % 5) * ((rows << lv) // 7 + 1)))
    out[6] = out[6][:4] + (out[6][4] // 3,) + out[6][5:]           # a truncated file: its bytes cannot hold its blocks
    out[13] = (0, 0, 0, 0, 8, 0, 0, 1)                              # not ACM
    out[14] = (0, 0, 0, 0, 0, 0, 0, 1)                              # empty
    out[20] = out[20][:5] + (2,) + out[20][6:]                      # room for two blocks only
    out[21] = out[21][:5] + (0,) + out[21][6:]                      # room for none
    out[22] = out[22][:7] + (0,)                                    # no mark buffer at all
    return out


def test_one_group_by_default():
    streams = mixed()
    T = layout(streams)
    check_properties(streams, T, 0)
    assert len(T["groups"]) == 1
    on = T["slots"]["on_dev"]
    assert not on[6] and not on[13] and not on[14] and not on[21] and not on[22]
    assert on[20] and T["slots"]["want_blocks"][20] == 2
    assert on.sum() == len(streams) - 5


def test_budget_cuts():
    streams = mixed()
    whole = layout(streams)
    cost = int(whole["groups"]["file_bytes"][0] + MARK * whole["groups"]["marks"][0])
    for budget in (cost, cost - 1, cost // 2, cost // 3, cost // 7, 4096, 1):
        T = layout(streams, budget)
        check_properties(streams, T, budget)
        assert (len(T["groups"]) == 1) == (budget >= cost)
    # a budget below every file: one-file groups
    T = layout(streams, 1)
    assert len(T["groups"]) == len(T["dev_ids"]) and np.all(T["groups"]["k_last"] - T["groups"]["k_first"] == 1)
    assert np.all(T["slots"]["file_off"] == 0) and np.all(T["slots"]["mark_off"] == 0)
    # one file alone above the budget sits in a group of its own between groups that respect it
    big = stream(9, 16, 400)
    streams = [stream(5, 4, 3)] * 5 + [big] + [stream(5, 4, 3)] * 5
    budget = big[4] // 2
    T = layout(streams, budget)
    check_properties(streams, T, budget)
    assert len(T["groups"]) == 3 and tuple(T["groups"]["k_last"] - T["groups"]["k_first"]) == (5, 1, 5)


def test_stream_count_cut():
    n = RANGE_MAX_STREAMS + 5
    streams = [stream(0, 1, 2)] * n
    T = layout(streams)
    check_properties(streams, T, 0)
    assert tuple(T["groups"]["k_last"] - T["groups"]["k_first"]) == (RANGE_MAX_STREAMS, 5)


def test_large_files_stay_on_the_host():
    """acmk_parse_supported: files below 256 MiB, 32-bit column counts.  The lengths are numbers: no image is read"""
    limit = 1 << 28
    streams = [stream(9, 16, 100, length=limit - 1), stream(9, 16, 100, length=limit), stream(9, 16, 100, length=5 * limit),
               (15, 1, 0xFFFFFFFF, 14, limit - 1, 1 << 17, 1, 1),       # blocks << level beyond 32 bits (and more blocks than the bytes hold)
               stream(5, 4, 3)]
    T = layout(streams, 1 << 40)
    check_properties(streams, T, 1 << 40)
    assert T["slots"]["on_dev"].tolist() == [1, 0, 0, 0, 1]
    assert T["host_ids"].tolist() == [1, 2, 3]


def test_short_files_stay_on_the_host():
    """a header that promises more blocks than the bytes can hold, with the room acm_batch_index_blocks gives it (as many blocks as the
    bytes could hold at the very most): not uploaded.  Asked for fewer blocks than that, the stream can still be clean"""
    level, rows, hb = 5, 8, 14
    whole = stream(level, rows, 40)
    length = hb + 225           # ten blocks of nothing but headers and codes, so nowhere near 40 real ones
    possible = ((length - hb) * 8 + 8) // (20 + (5 << level)) + 1
    assert 2 < possible < 40
    streams = [whole, whole[:4] + (length, possible) + whole[6:], whole[:4] + (length, 40) + whole[6:], whole[:4] + (length, 2) + whole[6:]]
    T = layout(streams)
    check_properties(streams, T, 0)
    assert T["slots"]["on_dev"].tolist() == [1, 0, 0, 1]
    assert T["slots"]["want_blocks"].tolist() == [40, possible, 40, 2]


def test_empty_batch():
    T = layout([])
    assert len(T["groups"]) == 0 and len(T["dev_ids"]) == 0 and tuple(T["totals"]) == (0, 0, 0, 0)
