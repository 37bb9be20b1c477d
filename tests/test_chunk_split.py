"""How a launch of the chunk kernel hands out its table (acmk_tile2m_split, libacm_amd/csrc/acm_kernel_geo.cpp): the first W *
static_per chunks are one static run per wavefront, the rest is nclaimed runs of run_chunks that the wavefronts claim in ascending
order.  Device-free: the function is pure host code, and so are the wavefront count and the override it rests on.

Checked for levels 8-12, under the compiled-in policy and under several policies set through acmk_tile2m_claim_config: static and
claimed runs cover every chunk exactly once and in order; below the threshold the split is the one contiguous run of ceil(ntiles /
W) chunks per wavefront that the kernel has always taken; the override hands back what it replaced and restores the defaults."""
import ctypes as C

import pytest

from libacm_amd import capi

CUS = 256
LEVELS = [8, 9, 10, 11, 12]
MIN_PER = 32                                    # ACM_CLAIM_MIN_PER: chunks per wavefront from which the compiled-in policy splits a table
PRIME = 1000003
# (chunks per claimed run, static share in thousandths)
OVERRIDES = [(2, 0), (3, 0), (3, 500), (16, 800), (64, 900), (1, 1000), (8, 1000), (5, 2000), (0, 500), (7, -1), (-1, 300)]


def L():
    lib = capi.lib()
    lib.acmk_tile2m_split.argtypes = [C.c_uint32, C.c_int, C.c_uint32] + [C.POINTER(C.c_uint32)] * 3
    lib.acmk_tile2m_claim_config.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.acmk_tile2m_claim_config.restype = None
    return lib


def split(lib, level, n):
    sp, rc, nc = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert lib.acmk_tile2m_split(level, CUS, n, C.byref(sp), C.byref(rc), C.byref(nc)) == 0
    return sp.value, rc.value, nc.value


def config(lib, run_chunks, permille):
    a, b = C.c_int(), C.c_int()
    lib.acmk_tile2m_claim_config(run_chunks, permille, C.byref(a), C.byref(b))
    return a.value, b.value


def sizes(W):
    return [0, 1, W - 1, W, W + 1, 3 * W, 3 * W + 1, PRIME, MIN_PER * W - 1, MIN_PER * W, MIN_PER * W + 1, 250 * W]


def static_runs_of_old(n, W):
    """the kernel's split before there were claimed runs: [w * per, min((w + 1) * per, n)) with per = ceil(n / W)"""
    per = -(-n // W)
    return [(w * per, min((w + 1) * per, n)) for w in range(W) if w * per < n]


def check_cover(n, W, sp, rc, nc):
    """every chunk exactly once, in order: the static runs one behind the other from 0, the claimed runs behind them"""
    if nc == 0:
        assert rc == 0 and sp == -(-n // W)
        runs = static_runs_of_old(n, W)
    else:
        assert rc > 0 and W * sp < n
        runs = [(w * sp, (w + 1) * sp) for w in range(W) if sp]
        base = W * sp
        assert nc == -(-(n - base) // rc)
        runs += [(base + k * rc, min(base + (k + 1) * rc, n)) for k in range(nc)]
        assert all(e - b == rc for b, e in runs[len(runs) - nc:-1])                # only the last claimed run may be shorter
    at = 0
    for b, e in runs:
        assert b == at and e > b, (b, e, at)
        at = e
    assert at == n


@pytest.mark.parametrize("level", LEVELS)
def test_defaults(level):
    lib = L()
    assert config(lib, -1, -1) is not None
    W = lib.acmk_tile2m_run_waves(level, CUS)
    assert W > 0 and W % CUS == 0
    for n in sizes(W):
        sp, rc, nc = split(lib, level, n)
        check_cover(n, W, sp, rc, nc)
        if n < MIN_PER * W:
            # below the threshold: today's formula, nothing claimed
            assert (sp, rc, nc) == (-(-n // W), 0, 0), (n, sp, rc, nc)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("run_chunks,permille", OVERRIDES)
def test_overrides(level, run_chunks, permille):
    lib = L()
    config(lib, -1, -1)
    W = lib.acmk_tile2m_run_waves(level, CUS)
    grid = lib.acmk_tile2m_grid(level, CUS)
    defaults = {n: split(lib, level, n) for n in sizes(W)}
    try:
        assert config(lib, run_chunks, permille) == (-1, -1)
        for n in sizes(W):
            sp, rc, nc = split(lib, level, n)
            check_cover(n, W, sp, rc, nc)
            if n < grid or run_chunks == 0:
                assert nc == 0                                  # fewer chunks than workgroups, or no claimed runs asked for: static
            elif nc:
                share = min(permille, 1000) if permille >= 0 else None
                if share is not None:
                    assert sp == n * share // 1000 // W
                if run_chunks > 0:
                    assert rc == run_chunks
            if run_chunks > 0 and permille == 0 and n >= grid and n > 0:
                assert sp == 0 and nc == -(-n // run_chunks)      # the whole table is claimed
    finally:
        old = config(lib, -1, -1)
    assert old == (run_chunks if run_chunks >= 0 else -1, permille if permille >= 0 else -1)
    # the defaults are back
    assert config(lib, -1, -1) == (-1, -1)
    assert {n: split(lib, level, n) for n in sizes(W)} == defaults


def test_levels_without_the_chunk_kernel():
    lib = L()
    sp, rc, nc = C.c_uint32(), C.c_uint32(), C.c_uint32()
    for level in (5, 7, 13, 14):
        assert lib.acmk_tile2m_run_waves(level, CUS) == 0
        assert lib.acmk_tile2m_split(level, CUS, 100000, C.byref(sp), C.byref(rc), C.byref(nc)) == -1
