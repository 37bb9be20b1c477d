"""The kernels' launch geometry as the host sees it (libacm_amd/csrc/acm_kernel_geo.h / .cpp): every acmk_* query that launches
nothing - tile rows, grids, first-pass depth, lead-in, packed slots, the chunk kernel's wavefronts and how they split a table, what the
device parser accepts and where its stripes and block ranges are cut - held to a table recorded from the commit BEFORE these answers
moved out of the kernels' translation units (tests/golden/kernel_geo.json, written by tests/golden/make_golden_kernel_geo.py).

Device-free.  The product library and the tuning library (-DACM_TUNING) are each asked in a fresh child process, the tuning library
once per setting of the switches it reads once per process: ACM_K3 unset / 0, ACM_K2M_G0 unset / 3 / 4.

The last case is the guard against a mixed build: a library whose kernels and whose planner were compiled from different geometries
(one of them with a -D flag that changes a tile) must be refused by acmhip_device_open."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_geo.json")

LEVELS = list(range(17))
CUS = [0, 1, 8, 256, 304]
# (library, environment): the switches are read once per process, so every setting is a process of its own
CONFIGS = [("shipped", {})] + [("tuning", dict(([("ACM_K3", k3)] if k3 else []) + ([("ACM_K2M_G0", g0)] if g0 else [])))
                               for k3 in ("", "0") for g0 in ("", "3", "4")]
SPLIT_LEVELS = [8, 9, 10, 11, 12]
SPLIT_CUS = [8, 256]
SPLIT_POLICIES = [(-1, -1), (2, 0), (3, 500), (5, 2000)]       # the compiled-in policy and three of tests/test_chunk_split.py's overrides
MIN_PER, PRIME = 32, 1000003


def config_name(lib, env):
    return ",".join([lib] + ["%s=%s" % kv for kv in sorted(env.items())])


def split_sizes(W):
    """tests/test_chunk_split.py::sizes"""
    return [0, 1, W - 1, W, W + 1, 3 * W, 3 * W + 1, PRIME, MIN_PER * W - 1, MIN_PER * W, MIN_PER * W + 1, 250 * W]


def record(L):
    """every answer of the loaded library L, as plain lists in a fixed order"""
    u32, u64, i = C.c_uint32, C.c_uint64, C.c_int
    for name, args, res in [("acmk_fused_tile_rows", [u32, i], i), ("acmk_fused_has_carry", [u32, i], i), ("acmk_fused_grid", [u32, i, i], i),
                            ("acmk_tile2_rows", [u32], i), ("acmk_tile2_grid", [u32, i], i), ("acmk_tile2m_rows", [u32], i),
                            ("acmk_tile2m_lead_in", [u32], i), ("acmk_tile2m_run_waves", [u32, i], i), ("acmk_tile2m_grid", [u32, i], i),
                            ("acmk_tile2m_stages", [u32], i), ("acmk_tile2p_rows", [u32], i), ("acmk_tile2p_group_rows", [u32], i),
                            ("acmk_tile2p_slots", [u32], i), ("acmk_tile2p_waves", [u32], i), ("acmk_tile2p_pad_shift", [u32], i),
                            ("acmk_plane_tile_rows", [], i), ("acmk_plane_grid", [i], i), ("acmk_tuning_build", [], i), ("acmk_fused_variants", [], i),
                            ("acmk_tile2m_split", [u32, i, u32] + [C.POINTER(u32)] * 3, i),
                            ("acmk_tile2m_claim_config", [i, i, C.POINTER(i), C.POINTER(i)], None),
                            ("acmk_parse_supported", [u32, u32, u64, u64], i), ("acmk_stripe_bound", [u32] * 3, u32), ("acmk_range_bound", [u32] * 4, u32)]:
        getattr(L, name).argtypes, getattr(L, name).restype = args, res
    nv = L.acmk_fused_variants()
    out = {"tuning_build": L.acmk_tuning_build(), "fused_variants": nv}
    out["fused_tile_rows"] = [[L.acmk_fused_tile_rows(lv, v) for lv in LEVELS] for v in range(-1, nv + 1)]
    out["fused_has_carry"] = [[L.acmk_fused_has_carry(lv, v) for lv in LEVELS] for v in range(-1, nv + 1)]
    out["fused_grid"] = [[[L.acmk_fused_grid(lv, v, cus) for cus in CUS] for lv in LEVELS] for v in range(-1, nv + 1)]
    for name in ("tile2_rows", "tile2m_rows", "tile2m_lead_in", "tile2m_stages", "tile2p_rows", "tile2p_group_rows", "tile2p_slots", "tile2p_waves",
                 "tile2p_pad_shift"):
        out[name] = [getattr(L, "acmk_" + name)(lv) for lv in LEVELS]
    for name in ("tile2_grid", "tile2m_run_waves", "tile2m_grid"):
        out[name] = [[getattr(L, "acmk_" + name)(lv, cus) for cus in CUS] for lv in LEVELS]
    out["plane_tile_rows"] = L.acmk_plane_tile_rows()
    out["plane_grid"] = [L.acmk_plane_grid(cus) for cus in CUS]
    # the split of a chunk table: [policy][level][cus] = the return code, or one (static_per, run_chunks, nclaimed) per size
    sp, rc, nc, a, b = u32(), u32(), u32(), i(), i()
    out["split"] = []
    for policy in SPLIT_POLICIES:
        L.acmk_tile2m_claim_config(policy[0], policy[1], None, None)
        rows = []
        for lv in SPLIT_LEVELS:
            for cus in SPLIT_CUS:
                W = L.acmk_tile2m_run_waves(lv, cus)
                if not W:
                    rows.append(L.acmk_tile2m_split(lv, cus, 100000, C.byref(sp), C.byref(rc), C.byref(nc)))
                    continue
                row = []
                for n in split_sizes(W):
                    assert L.acmk_tile2m_split(lv, cus, n, C.byref(sp), C.byref(rc), C.byref(nc)) == 0
                    row += [sp.value, rc.value, nc.value]
                rows.append(row)
        L.acmk_tile2m_claim_config(-1, -1, C.byref(a), C.byref(b))
        rows.append([a.value, b.value])                 # what the override hands back
        out["split"].append(rows)
    # the device parser
    lens = [0, 15, 16, 0x0FFFFFFF, 0x10000000]
    out["parse_supported"] = "".join(str(L.acmk_parse_supported(lv, rows, n, blocks)) for lv in LEVELS for rows in (0, 1) for n in lens
                                     for blocks in (0, 1, 250, (2 ** 32 >> lv) - 1, 2 ** 32 >> lv, (2 ** 32 >> lv) + 1))
    out["stripe_bound"] = [L.acmk_stripe_bound(n, s, S) for n in lens for S in range(1, 17) for s in range(S + 1)]
    out["range_bound"] = [L.acmk_range_bound(blocks, r, R, unit) for blocks in (0, 1, 250, (2 ** 32 >> 9) - 1, 2 ** 32 >> 9, (2 ** 32 >> 9) + 1)
                          for unit in (0, 1, 3, 16) for R in range(1, 17) for r in range(R + 1)]
    if os.environ.get("ACM_K3") or os.environ.get("ACM_K2M_G0"):
        # a setting of the switches: only what they choose, the build of a byte-plane level (the rest is in the recording without them)
        out = {k: v for k, v in out.items() if k.startswith("tile2m_") or k == "split"}
    return out


def record_in_child(path, env):
    """the answers of the library at `path` in a fresh process with `env` on top of the caller's (minus the switches it does not name)"""
    base = {k: v for k, v in os.environ.items() if k not in ("ACM_K3", "ACM_K2M_G0")}
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(base, ACM_HIP_LIB=path, **env), stdout=subprocess.PIPE, check=True)
    return json.loads(p.stdout)


def library_path(which):
    from libacm_amd import _build
    return _build.build_hip() if which == "shipped" else _build.build_tuning()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("lib,env", CONFIGS, ids=[config_name(*c) for c in CONFIGS])
def test_answers_are_the_recorded_ones(golden, lib, env):
    want = golden["configs"][config_name(lib, env)]
    got = record_in_child(library_path(lib), env)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


def test_the_table_reaches_what_it_is_for(golden):
    """the recording itself: the chunk kernel on and off, both depths of the matrix build, claimed runs, refused inputs"""
    cfg = golden["configs"]
    assert cfg["shipped"]["tile2m_stages"][8:13] == [6] * 5 and cfg["tuning,ACM_K3=0"]["tile2m_stages"][8:13] == [3, 3, 4, 4, 4]
    assert cfg["tuning,ACM_K2M_G0=4,ACM_K3=0"]["tile2m_stages"][8:10] == [4, 4] and cfg["tuning,ACM_K2M_G0=3,ACM_K3=0"]["tile2m_stages"][10:13] == [3, 3, 3]
    assert sorted(set(cfg["shipped"]["tile2m_lead_in"])) == [1, 2, 3]
    assert cfg["shipped"]["fused_variants"] == 1 and cfg["tuning"]["fused_variants"] > 1
    assert any(row[k + 2] for row in cfg["shipped"]["split"][0][:-1] for k in range(0, len(row), 3))          # claimed runs under the default policy
    assert all(r == -1 for r in cfg["tuning,ACM_K3=0"]["split"][0][:-1])
    assert "0" in cfg["shipped"]["parse_supported"] and "1" in cfg["shipped"]["parse_supported"]


def test_a_mixed_build_is_refused(tmp_path):
    """The planner's half compiled with a flag that changes a chunk's geometry (-DACM_K3_DPP_HISTORY=0: levels 8 and 9 keep no rows, their
    lead-in is one chunk), linked with the regular kernels: the two exported digests differ and acmhip_device_open refuses the library with
    ACMHIP_ERR_ARG - before it looks for a device, so the refusal is the same on a machine without one."""
    from libacm_amd import _build, capi
    _build.build_hip()
    objs = [os.path.join(_build.LIB, os.path.basename(s) + ".o") for s in _build.HIP_SOURCES if s != "acm_kernel_geo.cpp"]
    assert all(os.path.exists(o) for o in objs)
    geo = str(tmp_path / "geo.o")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-DACM_K3_DPP_HISTORY=0", "-I", _build.INC, "-I", _build.CSRC, "-c",
                    os.path.join(_build.CSRC, "acm_kernel_geo.cpp"), "-o", geo], check=True)
    mixed = str(tmp_path / "mixed.so")
    subprocess.run([_build.HIPCC, "-shared", "-fPIC", "--offload-arch=" + _build.GFX, "-o", mixed] + objs + [geo, "-lpthread"], check=True)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--open"], env=dict(os.environ, ACM_HIP_LIB=mixed), stdout=subprocess.PIPE, check=True)
    got = json.loads(p.stdout)
    assert got["planner"] != got["kernels"]
    assert got["open"] == capi.ERR_ARG and "geometr" in got["error"], got
    # ... and the regular library's halves agree
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--open"], env=dict(os.environ, ACM_HIP_LIB=_build.build_hip()), stdout=subprocess.PIPE,
                       check=True)
    got = json.loads(p.stdout)
    assert got["planner"] == got["kernels"] and got["open"] != capi.ERR_ARG, got


def _child_open():
    L = C.CDLL(os.environ["ACM_HIP_LIB"])
    L.acmk_geo_digest.restype = L.acmk_geo_digest_kernels.restype = C.c_uint64
    L.acmhip_last_error.restype = C.c_char_p
    dev = C.c_void_p()
    rc = L.acmhip_device_open(0, None, C.byref(dev))
    out = {"planner": L.acmk_geo_digest(), "kernels": L.acmk_geo_digest_kernels(), "open": rc, "error": (L.acmhip_last_error() or b"").decode()}
    if rc == 0:
        L.acmhip_device_close(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        print(json.dumps(record(C.CDLL(os.environ["ACM_HIP_LIB"]))))
    elif sys.argv[1:] == ["--open"]:
        _child_open()
