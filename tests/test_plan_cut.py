"""The launch planner's host half (libacm_amd/csrc/acm_plan_cut.cpp), without a GPU.

acmk_plan_cut_visit() runs the cutter at a given number of compute units and shows every table a plan would upload.  Three kinds of check
over one list of cases:

  * equality: the SHA-256 of every table, the return code and the error text equal what the planner of the commit named in
    tests/golden/plan_cut.json produced for the same case (recorded from that commit's code by tests/golden/make_golden_plan_cut.py
    through the instrumentation in profiles/plan_cut_parent_seam.patch; the fixture keeps them hashed once more, see recording());
  * coverage: the case list reaches every table, every record flag and both flavours of every choice (a condition on the list, asserted
    by the recorder on the recorded planner's output and here again);
  * properties of the records themselves: the emitted PCM is tiled exactly once, form_rows agrees with the second-form records,
    samples are counted, patches land inside the plane.

A second list, limit_cases(), is not held to the recording (the recorded planner wrapped there): header indices and pair-table entries
at 2^32 - 1, 2^32 and 2^32 + 1 are either exact in every table or refused (test_table_limits_are_refused_not_wrapped).

Two guards inside the cutter's cut_lean() have no case: "a window on the lean kernels starts on a tile boundary of a stream with a
byte-plane form" and "a window on the lean kernel of level L needs N rows in front".  Its only caller that passes a window (plain fused
streams, levels 5-12) checks the boundary and the form before it calls, and the one build whose lead-in is longer than a tile is level
14, which only ever comes from row 0.  They stay as guards against a future caller.  The "internal: H1 patch lands ..." check is an
assertion on the cutter's own arithmetic and has no case either.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np

from libacm_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_cut.json")

FORM_PACKED, FORM_BYTEPLANE = 0, 1
TILE_FRESH, TILE_DISCARD, TILE_ROW1, TILE_ODD, TILE_ONEBLOCK = 1, 2, 4, 8, 16
FLAG_SETS = {
    "auto": capi.PLAN_AUTO, "stagewise": capi.PLAN_STAGEWISE, "no_lean": capi.PLAN_NO_LEAN, "lean_always": capi.PLAN_LEAN_ALWAYS,
    "force_halo": capi.PLAN_FORCE_HALO, "force_carry": capi.PLAN_FORCE_CARRY, "form_only": capi.PLAN_FORM_ONLY,
    "lean_always_form_only": capi.PLAN_LEAN_ALWAYS | capi.PLAN_FORM_ONLY,
}
CUS = (2, 256)
TABLE_NAMES = {"streams", "tiles", "tiles_extra", "tiles2", "tiles2p", "tiles2p_plain", "tiles2m", "tiles2m_plain", "small_list",
               "prefix_list", "prefix_tiles", "sw_list", "sw_all", "patches", "form_rows"}

DEV_STREAM = np.dtype([("idx_off", "<u8"), ("hdr_off", "<u8"), ("pcm_off", "<u8"), ("n_emit", "<u8"), ("scratch_off", "<u8"),
                       ("level", "<u4"), ("rows", "<u4"), ("nrows", "<u4"), ("row_begin", "<u4"), ("halo_row", "<u4"), ("pad", "<u4")])
TILE = np.dtype([("stream", "<u4"), ("row0", "<i4"), ("flags", "<u4"), ("pad", "<u4")])
TILE2 = np.dtype([("idx_off", "<u8"), ("pcm_off", "<u8"), ("hdr_blk", "<u4"), ("rowpos", "<u4"), ("magic", "<u4"), ("flags", "<u4")])
DEV_PATCH = np.dtype([("dst", "<u8"), ("value", "<i4"), ("pad", "<u4")])
DTYPES = {"streams": DEV_STREAM, "tiles": TILE, "tiles_extra": TILE, "prefix_tiles": TILE, "tiles2": TILE2, "tiles2p": TILE2,
          "tiles2p_plain": TILE2, "tiles2m": TILE2, "tiles2m_plain": TILE2, "small_list": "<u4", "prefix_list": "<u4", "sw_list": "<u4",
          "sw_all": "<u4", "patches": DEV_PATCH, "form_rows": "<u8", "stats": "<u8"}
KIND_FUSED, KIND_SMALL, KIND_PREFIX, KIND_STAGEWISE = 0, 1, 2, 3

VISIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_size_t)


def _lib():
    L = capi.lib()
    L.acmk_plan_cut_visit.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, VISIT, C.c_void_p]
    L.acmhip_set_error_text.argtypes = [C.c_char_p]
    L.acmhip_set_error_text.restype = None
    for f in ("acmk_fused_tile_rows", "acmk_tile2_rows", "acmk_tile2p_rows", "acmk_tile2p_slots", "acmk_tile2m_rows", "acmk_plane_tile_rows"):
        getattr(L, f).restype = C.c_int
    return L


# ---------------------------------------------------------------------------------------------------------------- the case list

class Case:
    def __init__(self, name, cus, flags, descs, packed=None, patches=(), raw_n=None, null_streams=False, null_patches=False):
        self.name, self.cus, self.flags, self.descs, self.packed, self.patches = name, cus, flags, descs, packed, patches
        self.raw_n, self.null_streams, self.null_patches = raw_n, null_streams, null_patches


class Batch:
    """descriptors laid out one behind the other in the arenas, the way a stager would: offsets are multiples of 8"""

    def __init__(self, L):
        self.L, self.descs, self.packed = L, [], []
        self.idx = self.hdr = self.pcm = self.chunk = 0

    def add(self, level, rows, nrows, row_begin, n_emit, form=None, short_by=0):
        L = self.L
        self.descs.append(capi.StreamDesc(self.idx, self.hdr, self.pcm, n_emit, level, rows, nrows, row_begin))
        self.idx += ((nrows << level) + 7) & ~7
        self.hdr += (nrows + rows - 1) // max(rows, 1)
        self.pcm += ((n_emit + 7) & ~7) + 8 * (len(self.descs) % 2)
        if form == FORM_PACKED:
            t = L.acmk_tile2p_rows(level)
            ntiles = max(nrows // t - short_by, 0) if t else 3
            self.packed.append(capi.PackedStream(self.chunk, ntiles, FORM_PACKED))
            self.chunk += ntiles * max(L.acmk_tile2p_slots(level), 1)
        elif form is not None:          # the byte-plane form, or a form code the library does not know
            t = L.acmk_tile2m_rows(level)
            ntiles = max((nrows + t - 1) // t - short_by, 1) if t else 3
            self.packed.append(capi.PackedStream(self.chunk, ntiles, form))
            self.chunk += nrows // 2 + 1
        else:
            self.packed.append(capi.PackedStream(0, 0, 0))
        return len(self.descs) - 1

    def case(self, name, cus, flags, patches=(), with_packed=None):
        use = any(p.ntiles for p in self.packed) if with_packed is None else with_packed
        return Case(name, cus, flags, self.descs, self.packed if use else None, patches)


def _unit(L, level):
    """the tile a level's streams are measured in: the lean kernels' tile, else the fused kernel's payload rows, else 4 rows"""
    if L.acmk_tile2_rows(level):
        return L.acmk_tile2_rows(level)
    return L.acmk_fused_tile_rows(level, 0) - 2 if L.acmk_fused_tile_rows(level, 0) else 4


def _sweep(L, level, form):
    """one level: rows of 1, 2, an odd height and 4095; row_begin 0, one tile (a lead-in that is the stream's first tile), two tiles, one
    row off that; n_emit 0, whole tiles exactly, ragged"""
    b, u = Batch(L), _unit(L, level)
    for rows in (1, 2, 7, 4095):
        for row_begin in (0, u, 2 * u, 2 * u + 1):
            nrows = row_begin + 3 * u + 8
            for n_emit in (0, (3 * u) << level, ((2 * u + u // 2 + 1) << level) + 5):
                b.add(level, rows, nrows, row_begin, n_emit, form)
    return b


def _mixed(L, count, seed):
    """a few hundred streams of every level and form, sizes from a fixed linear congruential sequence"""
    state = [seed]

    def rnd(n):
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (state[0] >> 33) % n
    b = Batch(L)
    for k in range(count):
        level = (k * 7 + rnd(3)) % 16
        u = _unit(L, level)
        row_begin = (0, 0, u, 2 * u, 3 * u + 1)[rnd(5)]
        emit_rows = rnd(5 * u) + 1
        nrows = row_begin + emit_rows + rnd(4)
        n_emit = (0, emit_rows << level, max((emit_rows << level) - rnd(1 << level) - 1, 1))[rnd(3) if rnd(8) else 0]
        form = (None, FORM_PACKED if 6 <= level <= 9 else None, FORM_BYTEPLANE if 7 <= level <= 14 else None)[rnd(3)]
        b.add(level, (1, 2, 5, 64, 4095)[rnd(5)], nrows, row_begin, n_emit, form)
    return b


def _patched(L):
    """H1 patches: inside a tile, inside the two halo rows of the next tile, behind the last emitted row, on a windowed stream, on a
    stream that emits nothing, on level-13 / 15 streams (planes carry scaled values), on a small-level stream (stage-wise), outside the
    staged rows; clean streams beside them"""
    b, patches = Batch(L), []

    def patch(stream, level, row, col, value):
        patches.append(capi.Patch((row << level) + col, value, stream))
    for level in (5, 9, 12):
        t = L.acmk_fused_tile_rows(level, 0) - 2
        a = b.add(level, 3, 3 * t + 5, 0, ((2 * t + 3) << level) - 7)
        patch(a, level, t + t // 2, 3, 1000 + level)
        patch(a, level, t - 1, 0, -2000 - level)
        patch(a, level, 3 * t + 2, 1, 77)
        w = b.add(level, 4095, 4 * t + 9, t + 1, (2 * t) << level)
        patch(w, level, t + 2, 5, 31000)
        patch(w, level, 1, 0, 5)                    # in front of the window's halo rows: nobody sees it
        b.add(level, 2, 2 * t + 2, 0, (2 * t) << level)
        z = b.add(level, 1, 8, 2, 0)
        patch(z, level, 3, 0, 9)
    for level, value in ((13, 1234), (15, -4321)):
        p = b.add(level, 2, 12, 0, (11 << level) + 1)
        patch(p, level, 5, 17, value)
        patch(p, level, 12, 0, 1)                   # behind the staged rows
        w = b.add(level, 1, 16, 6, 9 << level)
        patch(w, level, 2, 0, 3)                    # in front of the halo rows
        patch(w, level, 7, 1, value + 1)
        b.add(level, 7, 10, 0, 10 << level)
    s = b.add(3, 1, 40, 0, 300)
    patch(s, 3, 4, 1, -5)
    b.add(3, 1, 40, 4, 200)
    return b, (capi.Patch * len(patches))(*patches)


def _errors(L):
    good = dict(level=9, rows=3, nrows=40, row_begin=0, n_emit=40 << 9)
    out = []
    for tag, change in (("level_16", dict(level=16)), ("rows_0", dict(rows=0)), ("rows_4096", dict(rows=4096)),
                        ("row_begin_past_nrows", dict(row_begin=41, n_emit=0)), ("n_emit_past_rows", dict(n_emit=(40 << 9) + 1)),
                        ("n_emit_past_window", dict(row_begin=8, n_emit=(32 << 9) + 1))):
        b = Batch(L)
        b.add(9, 3, 40, 0, 1000)
        b.add(**dict(good, **change))
        out.append(b.case("err_desc_" + tag, 2, 0))
    for tag, field in (("idx_off", "idx_off"), ("pcm_off", "pcm_off")):
        b = Batch(L)
        b.add(**good)
        setattr(b.descs[0], field, 4)
        out.append(b.case("err_desc_" + tag, 2, 0))
    b = Batch(L)
    b.add(**good)
    out.append(b.case("err_patch_stream", 2, 0, patches=(capi.Patch * 2)(capi.Patch(5, 1, 0), capi.Patch(5, 1, 1))))
    for tag, level, form, short_by, row_begin in (("form_code", 9, 2, 0, 0), ("packed_tiles", 9, FORM_PACKED, 1, 0),
                                                  ("byteplane_tiles", 9, FORM_BYTEPLANE, 1, 0), ("byteplane_window_tiles", 9, FORM_BYTEPLANE, 2, 16),
                                                  ("form_code_13", 13, 7, 0, 0), ("byteplane_tiles_14", 14, FORM_BYTEPLANE, 1, 0)):
        b = Batch(L)
        b.add(level, 2, 20, 0, 20 << level, FORM_BYTEPLANE if level < 13 else None)
        b.add(level, 2, row_begin + 64, row_begin, 64 << level, form, short_by)
        out.append(b.case("err_" + tag, 2, capi.PLAN_LEAN_ALWAYS))
    b = Batch(L)
    b.add(**good)
    out.append(Case("err_null_streams", 2, 0, b.descs, null_streams=True))
    out.append(Case("err_null_patches", 2, 0, b.descs, patches=(capi.Patch * 1)(capi.Patch(5, 1, 0)), null_patches=True))
    out.append(Case("err_n_past_32_bits", 2, 0, b.descs, raw_n=(1 << 32) + 1))
    return out


def build_cases(L):
    cases = []
    for cus in CUS:
        for fname, flags in FLAG_SETS.items():
            for level in range(16):
                forms = [("plain", None)] + ([("packed", FORM_PACKED)] if 6 <= level <= 9 else []) + \
                        ([("byteplane", FORM_BYTEPLANE)] if 7 <= level <= 14 else [])
                for tag, form in forms:
                    cases.append(_sweep(L, level, form).case("sweep_cus%d_%s_l%d_%s" % (cus, fname, level, tag), cus, flags))
        for fname in ("auto", "lean_always", "no_lean", "form_only", "stagewise"):
            cases.append(_mixed(L, 300, 12345).case("mixed_cus%d_%s" % (cus, fname), cus, FLAG_SETS[fname]))
        for fname in ("auto", "stagewise", "no_lean", "lean_always", "force_carry"):
            b, patches = _patched(L)
            cases.append(b.case("patched_cus%d_%s" % (cus, fname), cus, FLAG_SETS[fname], patches))
        # levels 13 / 14 with a handful of whole tiles: below the 8 * grid threshold even on two compute units; one stream, packed array absent
        for level in (13, 14):
            b = Batch(L)
            b.add(level, 2, 3 * _unit(L, level) + 1, 0, (3 * _unit(L, level) + 1) << level, FORM_BYTEPLANE)
            cases.append(b.case("few_tiles_cus%d_l%d" % (cus, level), cus, 0))
            cases.append(b.case("few_tiles_cus%d_l%d_no_forms" % (cus, level), cus, 0, with_packed=False))
    cases.append(Case("empty", 2, 0, []))
    cases += _errors(L)
    assert len({c.name for c in cases}) == len(cases)
    return cases


E32 = 1 << 32
PAIR_READ_SLACK = 32            # entries the pair table is readable past its last one (include/acm_hip.h: acmhip_plan_bind_mform)
LIMIT_FLAVOURS = (("lean", capi.PLAN_LEAN_ALWAYS, None), ("byteplane", capi.PLAN_LEAN_ALWAYS, FORM_BYTEPLANE),
                  ("byteplane_form_only", capi.PLAN_LEAN_ALWAYS | capi.PLAN_FORM_ONLY, FORM_BYTEPLANE), ("packed", capi.PLAN_LEAN_ALWAYS, FORM_PACKED),
                  ("no_lean", capi.PLAN_NO_LEAN, FORM_BYTEPLANE), ("stagewise", capi.PLAN_STAGEWISE, FORM_PACKED), ("auto", capi.PLAN_AUTO, None))


def _limit_batch(L, level, form, rows=3):
    """a near stream, then the one whose offset a case moves: from row 0 (lean, byte-plane and packed tiles, a ragged rest), and
    (byte-plane form, levels up to 12) a window of it from a tile boundary"""
    b, u = Batch(L), _unit(L, level)
    b.add(level, 2, 2 * u + 1, 0, (2 * u + 1) << level, form)
    b.add(level, rows, 3 * u + 5, 0, ((3 * u + 4) << level) + 3, form)
    if form == FORM_BYTEPLANE and level <= 12:
        b.add(level, rows, 3 * u + 5, u, (2 * u) << level, form)
        b.descs[2].idx_off, b.descs[2].hdr_off = b.descs[1].idx_off, b.descs[1].hdr_off
        b.packed[2].chunk_off = b.packed[1].chunk_off
    return b


def form_entries(L, d, p):
    """table entries a stream's second staged form takes (acmhip_packed_stream)"""
    if p.form == FORM_PACKED:
        return p.ntiles * L.acmk_tile2p_slots(d.level)
    return p.ntiles * max(L.acmk_tile2m_rows(d.level), 0) // 2 + 1


def limit_cases(L):
    """-> [(case, the same case with the moved offsets near, what moved, by how much, whether include/acm_hip.h allows it)]: hdr_off + blocks
    and chunk_off + a stream's entries at 2^32 - 1, 2^32 and 2^32 + 1 (and chunk_off of a byte-plane stream with the pair table's read
    slack behind it at 2^32 and one past), for plans that cut lean, byte-plane and packed records and for plans that do not.  Not part of
    build_cases(): that list is held to a planner recorded before these limits existed, which wrapped."""
    out = []
    for level, flavours in ((9, LIMIT_FLAVOURS), (11, LIMIT_FLAVOURS[:3]), (14, LIMIT_FLAVOURS[1:2]), (3, LIMIT_FLAVOURS[-1:])):
        for fname, flags, form in flavours:
            near = _limit_batch(L, level, form)
            blocks = (near.descs[1].nrows + near.descs[1].rows - 1) // near.descs[1].rows
            points = [("hdr_off", E32 + k - blocks, k <= 0) for k in (-1, 0, 1, blocks, blocks + 8)]       # (the last two: hdr_off itself at and past 2^32)
            if form is not None:
                ent = form_entries(L, near.descs[1], near.packed[1])
                slack = PAIR_READ_SLACK if form == FORM_BYTEPLANE else 0
                points += [("chunk_off", E32 + k - ent, form == FORM_PACKED or k + slack <= 0) for k in sorted({-1, 0, 1, -slack, 1 - slack})]
            for what, value, allowed in points:
                far = _limit_batch(L, level, form)
                base = getattr(near.descs[1], what) if what == "hdr_off" else near.packed[1].chunk_off
                for k in range(1, len(far.descs)):
                    setattr(far.descs[k] if what == "hdr_off" else far.packed[k], what, value)
                name = "limit_l%d_%s_%s_%d" % (level, fname, what, value)
                out.append((far.case(name, 2, flags), near.case(name + "_near", 2, flags), what, value - base, allowed))
    assert len({c[0].name for c in out}) == len(out)
    return out


# ---------------------------------------------------------------------------------------------------------------- running a case

def run_case(L, case):
    """-> {"rc", "err", "tables": {"name@level": bytes}}"""
    tables = {}

    def visit(_ctx, name, level, data, elem_bytes, count):
        key = "%s@%d" % (name.decode(), level)
        assert key not in tables, key
        tables[key] = C.string_at(data, elem_bytes * count)
    n = len(case.descs)
    arr = (capi.StreamDesc * max(n, 1))(*case.descs)
    pk = (capi.PackedStream * max(n, 1))(*case.packed) if case.packed is not None else None
    L.acmhip_set_error_text(b"")
    rc = L.acmk_plan_cut_visit(case.cus, None if case.null_streams else arr, case.raw_n if case.raw_n is not None else n, pk,
                               None if case.null_patches or not len(case.patches) else case.patches, len(case.patches),
                               case.flags, VISIT(visit), None)
    return {"rc": rc, "err": L.acmhip_last_error().decode(), "tables": tables}


def digest(result):
    return {"rc": result["rc"], "err": result["err"], "tables": {k: hashlib.sha256(v).hexdigest() for k, v in sorted(result["tables"].items())}}


def fingerprint(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()


def recording(cases, results):
    """What the fixture keeps of a planner's answers.  sha256_of_all is the SHA-256 over every case's name, return code, error text and
    the SHA-256 of each of its tables (the equality that is asserted); case_sha256_16 - the first 16 hex digits of each case's own
    fingerprint, in the order of the case list - says WHICH case differs; errors shows codes and texts of the failing cases in plain"""
    each = [[c.name, digest(r)] for c, r in zip(cases, results)]
    return {"sha256_of_all": fingerprint(each), "errors": {name: [d["rc"], d["err"]] for name, d in each if d["rc"] != 0},
            "case_sha256_16": [fingerprint(e)[:16] for e in each]}


def decode(result):
    """{"name@level": bytes} -> {(name, level): numpy records}"""
    out = {}
    for key, raw in result["tables"].items():
        name, level = key.split("@")
        out[(name, int(level))] = np.frombuffer(raw, dtype=DTYPES[name])
    return out


def groups_of(stats_words):
    """the tail of the stats table: (plane_elems, sw_max_elems, need_sink, [(kind, level, carry, max_elems, max_emit, patched, stages)])"""
    w = [int(x) for x in stats_words]
    plane, sw_max, sink, ngroups = w[5:9]
    assert len(w) == 9 + 7 * ngroups
    return plane, sw_max, sink, [tuple(w[9 + 7 * k:16 + 7 * k]) for k in range(ngroups)]


# ---------------------------------------------------------------------------------------------------------------- coverage

def coverage(cases, results):
    """what the case list reaches, as {condition: bool}; every one must hold"""
    seen = {}

    def mark(what, ok=True):
        seen[what] = seen.get(what, False) or bool(ok)
    for what in ["table " + t for t in sorted(TABLE_NAMES)] + \
            ["tiles2m fresh", "tiles2m discard", "tiles2m fresh|discard", "tiles2m row1", "tiles2m odd", "tiles2m oneblock set",
             "tiles2m oneblock clear", "tiles2m finer than its plain twin", "fused carry", "fused halo", "prefix carry", "prefix halo",
             "prefix patched", "patch value shifted", "error code"]:
        mark(what, False)
    for case, res in zip(cases, results):
        mark("error code", res["rc"] == capi.ERR_ARG)
        tabs = decode(res)
        for (name, level), rec in tabs.items():
            if name in TABLE_NAMES:
                mark("table " + name)
            if name == "tiles2m":
                f = rec["flags"]
                mark("tiles2m fresh", ((f & 3) == TILE_FRESH).any())
                mark("tiles2m discard", ((f & 3) == TILE_DISCARD).any())
                mark("tiles2m fresh|discard", ((f & 3) == 3).any())
                mark("tiles2m row1", (f & TILE_ROW1).any())
                mark("tiles2m odd", (f & TILE_ODD).any())
                mark("tiles2m oneblock set", (f & TILE_ONEBLOCK).any())
                mark("tiles2m oneblock clear", ((f & TILE_ONEBLOCK) == 0).any())
                plain = tabs.get(("tiles2m_plain", level))
                mark("tiles2m finer than its plain twin", plain is not None and len(rec) > len(plain))
            if name == "patches":
                given = {p.value for p in case.patches}
                mark("patch value shifted", any(int(v) not in given for v in rec["value"]))
        if ("stats", 0) in tabs:
            for kind, _level, carry, _me, _mm, patched, _stages in groups_of(tabs[("stats", 0)])[3]:
                if kind == KIND_FUSED:
                    mark("fused carry" if carry else "fused halo")
                if kind == KIND_PREFIX:
                    mark("prefix carry" if carry else "prefix halo")
                    mark("prefix patched", patched)
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


def test_equal_to_the_recorded_planner():
    _, cases, results = _all()
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["recorded_from"], "the fixture names the commit whose planner it was recorded from"
    got = recording(cases, results)
    # no case is left out: the fixture has one fingerprint per case of the list, and names are part of what is hashed
    assert len(got["case_sha256_16"]) == len(golden["case_sha256_16"]) == len(cases)
    wrong = [(c.name, digest(r)) for c, r, a, b in zip(cases, results, got["case_sha256_16"], golden["case_sha256_16"]) if a != b]
    assert not wrong, "%d of %d cases differ from the recorded planner, first: %r" % (len(wrong), len(cases), wrong[:2])
    assert got["errors"] == golden["errors"]
    assert got["sha256_of_all"] == golden["sha256_of_all"]


def test_case_list_covers_the_planner():
    _, cases, results = _all()
    missing = [what for what, ok in coverage(cases, results).items() if not ok]
    assert not missing, missing


def _intervals(L, case, tabs):
    """[start, end) of PCM every record and list entry of the cut emits"""
    streams = tabs[("streams", 0)]
    _, _, _, groups = groups_of(tabs[("stats", 0)])
    carry_of = {(kind, level): carry for kind, level, carry, *_ in groups}
    out = []

    for (name, level), rec in tabs.items():
        if name in ("tiles", "tiles_extra", "prefix_tiles"):
            carry = name != "tiles_extra" and carry_of[(KIND_PREFIX if name == "prefix_tiles" else KIND_FUSED, level)]
            full = L.acmk_plane_tile_rows() if name == "prefix_tiles" else L.acmk_fused_tile_rows(level, 0)
            for t in rec:
                if t["flags"] & TILE_DISCARD:
                    continue
                s = streams[t["stream"]]
                lv, payload = int(s["level"]), full - (0 if carry else 2)
                at = (int(t["row0"]) - int(s["row_begin"])) << lv
                out.append((int(s["pcm_off"]) + at, int(s["pcm_off"]) + min(at + (payload << lv), int(s["n_emit"]))))
        elif name in ("tiles2", "tiles2p", "tiles2m"):
            rows = {"tiles2": L.acmk_tile2_rows, "tiles2p": L.acmk_tile2p_rows, "tiles2m": L.acmk_tile2m_rows}[name](level)
            for t in rec[(rec["flags"] & TILE_DISCARD) == 0]:
                out.append((int(t["pcm_off"]), int(t["pcm_off"]) + (rows << level)))
        elif name in ("small_list", "sw_list"):     # (a prefix_list entry emits through the tiles of its plane stream: counted there)
            for s in streams[rec]:
                out.append((int(s["pcm_off"]), int(s["pcm_off"]) + int(s["n_emit"])))
    return out


def _merged(intervals):
    out = []
    for a, b in sorted(i for i in intervals if i[1] > i[0]):
        assert not out or a >= out[-1][1], "PCM [%d, %d) is emitted twice" % (a, min(b, out[-1][1]))
        if out and a == out[-1][1]:
            out[-1][1] = b
        else:
            out.append([a, b])
    return out


def test_records_tile_the_pcm_exactly_once():
    L, cases, results = _all()
    checked = 0
    for case, res in zip(cases, results):
        if res["rc"] != 0 or not case.descs:
            continue
        tabs = decode(res)
        want = _merged((d.pcm_off, d.pcm_off + d.n_emit) for d in case.descs)
        assert _merged(_intervals(L, case, tabs)) == want, case.name
        # the int16 twins of the second-form records cover the same PCM as the records they stand in for
        for (name, level), rec in tabs.items():
            if name in ("tiles2p_plain", "tiles2m_plain"):
                form = tabs[(name[:-6], level)]
                twin_rows, form_rows = L.acmk_tile2_rows(level), (L.acmk_tile2p_rows if name == "tiles2p_plain" else L.acmk_tile2m_rows)(level)
                live = lambda r, rows: _merged((int(t["pcm_off"]), int(t["pcm_off"]) + (rows << level)) for t in r[(r["flags"] & TILE_DISCARD) == 0])
                assert live(rec, twin_rows) == live(form, form_rows), case.name
        checked += 1
    assert checked > 400


def test_form_rows_samples_and_patches():
    L, cases, results = _all()
    for case, res in zip(cases, results):
        if res["rc"] != 0 or not case.descs:
            continue
        tabs = decode(res)
        stats = tabs[("stats", 0)]
        assert int(stats[0]) == sum(d.n_emit for d in case.descs), case.name
        covered = 0
        for (name, level), rec in tabs.items():
            if name == "tiles2p":
                covered += len(rec) * L.acmk_tile2p_rows(level)
            if name == "tiles2m":
                covered += int(((rec["flags"] & TILE_DISCARD) == 0).sum()) * L.acmk_tile2m_rows(level)
        assert int(tabs.get(("form_rows", 0), np.zeros(1, "<u8")).sum()) == covered, case.name
        plane = groups_of(stats)[0]
        if ("patches", 0) in tabs:
            assert (tabs[("patches", 0)]["dst"] < plane).all(), case.name


def test_table_limits_are_refused_not_wrapped():
    """include/acm_hip.h: header indices and the byte-plane form's pair-table entries end below 2^32 (AcmTile2.hdr_blk has 32 bits, the
    byte-plane kernels read the pair table at a 32-bit index, 32 entries of read slack included); the packed chunk table is indexed in
    64 bits.  A plan whose stream stays within that equals, table by table, the plan of the same batch with the stream's offset near 0,
    every header index / table entry moved by exactly the 64-bit difference; one that does not is ACMHIP_ERR_ARG with a message that
    names the stream - whichever kernel family the plan would have used - and emits no table"""
    L = _lib()
    cases = limit_cases(L)
    moved_fields = {"hdr_off": {"streams": "hdr_off", "tiles2": "hdr_blk", "tiles2p": "hdr_blk", "tiles2p_plain": "hdr_blk", "tiles2m": "hdr_blk",
                                "tiles2m_plain": "hdr_blk"},
                    "chunk_off": {"tiles2p": "idx_off", "tiles2m": "idx_off"}}
    seen = set()
    for far, near, what, shift, allowed in cases:
        res = run_case(L, far)
        if not allowed:
            assert res["rc"] == capi.ERR_ARG and not res["tables"], far.name
            assert res["err"].startswith("stream 1: ") and what in res["err"], (far.name, res["err"])
            seen.add((what, False))
            continue
        assert res["rc"] == 0, (far.name, res["err"])
        ref = run_case(L, near)
        assert ref["rc"] == 0 and res["tables"].keys() == ref["tables"].keys(), far.name
        base = near.descs[1].hdr_off if what == "hdr_off" else near.packed[1].chunk_off
        assert base > 0
        ft, nt = decode(res), decode(ref)
        for (name, level), want in nt.items():
            got = ft[(name, level)]
            assert got.shape == want.shape, (far.name, name)
            field = moved_fields[what].get(name)
            if field is None:
                assert got.tobytes() == want.tobytes(), (far.name, name)
                continue
            for f in want.dtype.names:
                if f != field:
                    assert np.array_equal(got[f], want[f]), (far.name, name, f)
            w64 = want[field].astype(np.uint64)
            moved = w64 >= np.uint64(base)
            assert moved.any() and not moved.all(), (far.name, name)
            w64[moved] += np.uint64(shift)
            assert np.array_equal(got[field].astype(np.uint64), w64), "%s: %s.%s is not the 64-bit value" % (far.name, name, field)
            if name == "tiles2m" and what == "chunk_off":       # as the kernels read it: 32 bits, whole groups of entries
                assert int(w64.max()) + PAIR_READ_SLACK < E32
            seen.add((what, name))
    assert {("hdr_off", False), ("chunk_off", False)} <= seen
    assert {(w, n) for w, names in moved_fields.items() for n in names} <= seen, seen
