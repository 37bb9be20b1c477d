"""One call of the dense family described without a device (libacm_amd/csrc/acm_dense_call.h, header only): what was asked, the layouts of its
parts, the map of the H_JOBS / D_JOBS arenas and the tables as they go up.  No device here.

tests/native/dense_call.cpp holds acm_jobs_map() to a table worked out by hand - parser bytes 0, 1, 64 and 65, the five call shapes,
section sizes 0, 16 and 72 -, DenseCall::pack() to the spans and the bytes of one tiny call per shape inside a poisoned arena, and
acm_dense_call() to its four error texts and to the first of two.  Built with AddressSanitizer and UBSan, as a program of its own.
The driver's side of the seam is held here by its text: one decode_windows_dense without defaulted or bool parameters, no offset
arithmetic in acm_batch_windows.cpp, no private keywords or getattr dispatch in capi.py."""
import inspect
import os
import re
import subprocess

from libacm_amd import _build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINKED = ("acm_dense_layout.cpp", "acm_overlay_layout.cpp", "acm_fir_layout.cpp", "acm_feat_layout.cpp",
          "acm_resample_layout.cpp", "acm_window_layout.cpp", "acm_kernel_geo.cpp")


def test_call_against_the_tables_by_hand(tmp_path):
    exe = str(tmp_path / "dense_call")
    src = [os.path.join(ROOT, "tests", "native", "dense_call.cpp")] + [os.path.join(_build.CSRC, f) for f in LINKED]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", _build.INC, "-I", _build.CSRC, "-o", exe] + src + ["-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"dense_call: (\d+) map cases", r.stdout)
    assert m and int(m.group(1)) >= 40, r.stdout[-1000:]
    assert [s for s in ("dense", "overlay", "overlay_fir", "features", "features_fir") if "dense_call: pack %s\n" % s in r.stdout] == \
        ["dense", "overlay", "overlay_fir", "features", "features_fir"]
    assert "dense_call: refusals\n" in r.stdout and r.stdout.endswith("ok\n")


def _code(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(_build.CSRC, name)).read(), flags=re.S)


def test_the_description_knows_no_device():
    assert "hip" not in _code("acm_dense_call.h").lower().replace("acm_hip.h", "").replace("acmhip_", "")


def test_the_driver_keeps_no_arena_arithmetic():
    src = _code("acm_batch_windows.cpp")
    assert src.count("int decode_windows_dense(") == 1 and src.count("decode_windows_dense(dev, items, n, index, wins, nwin, opts_in, ask, tm)") == 4
    sig = src[src.index("int decode_windows_dense("):]
    sig = sig[:sig.index("{")]
    assert "bool" not in sig and "=" not in sig
    ctor = src[src.index("WinRun(acmhip_device"):]
    ctor = ctor[:ctor.index(")")]
    assert ctor.count("DenseCall") == 1 and "=" not in ctor and "Layout *" not in ctor
    for gone in ("overlay_off", "fir_off", "feat_off", "jobs_bytes()", "round_up", "table_off"):
        assert gone not in src, gone
    assert src.count("hipEventElapsedTime") == 3
    # ... and the dense layout asks the map where its tables begin
    assert "round_up(L.job_arena_bytes()" not in _code("acm_dense_layout.h") + _code("acm_dense_layout.cpp")
    assert re.search(r"DenseLayout::table_off\(const WindowLayout &L\) const \{ return acm_jobs_map\(", _code("acm_dense_call.h"))


def test_capi_has_one_preamble_and_one_overlay_call():
    src = inspect.getsource(capi)
    assert not re.search(r"\b_fir\b|\b_feat\b", src) and "getattr(lib()" not in src
    assert src.count("_dense_options(") == 3 and src.count("_overlay_call(") == 4 and src.count("DENSE_PLANAR if planar") == 1
    assert "_fir" not in inspect.signature(capi.batch_decode_windows_overlay).parameters
    assert src.count("in enumerate(windows)") == 1
