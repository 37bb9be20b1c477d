"""The launch geometry of the dense kernels has one owner, libacm_amd/csrc/acm_dense_geo.h: sub-rows, units of 256 lanes and 8 samples,
the two refusals and the capped grid.  No device here.

tests/native/dense_geo.cpp asks dense_geo() for a table worked out by hand: sub-rows of 0, 7, 8, 2047 and 2048 samples have one unit
and 2056 have two; planar stereo doubles the work items; the energy launch's units are 2048 samples and no more; a cap of 0 is the
built-in 2^20, 1 to 3 hold and nothing raises it; units past 2^31 - 1 and work past 2^64 are refused.  Built with AddressSanitizer and
UBSan, as a program of its own."""
import os
import re
import subprocess

from libacm_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHERS = {"acm_dense.hip": 1, "acm_dense_mix.hip": 1, "acm_dense_resample.hip": 1, "acm_dense_speed.hip": 1, "acm_dense_overlay.hip": 2}


def test_geometry_against_the_table_by_hand(tmp_path):
    exe = str(tmp_path / "dense_geo")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", _build.INC, "-I", _build.CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "dense_geo.cpp")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"dense_geo: (\d+) cases", r.stdout)
    assert m and int(m.group(1)) >= 30, r.stdout[-1000:]


def test_every_launcher_asks_the_header():
    """the six launches of the five files take units, work and grid from dense_geo, and none keeps an expression of its own beside it"""
    for name, launches in LAUNCHERS.items():
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(_build.CSRC, name)).read(), flags=re.S)
        assert src.count("dense_geo(") == launches, name
        assert "acm_cap_value" not in src and not re.search(r"\b(nwork|units|grid) = ", src), name
    hdr = open(os.path.join(_build.CSRC, "acm_dense_geo.h")).read()
    assert "hip" not in re.sub(r"/\*.*?\*/", "", hdr, flags=re.S).lower()
