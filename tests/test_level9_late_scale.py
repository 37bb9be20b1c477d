"""Level 9 takes the power of two that puts its samples on a byte boundary in the LAST LDS pass (libacm_amd/csrc/acm_late_scale.h,
DESIGN.md 2): stage 7 of the cascade, kind P, multiplies by 2^7 through the shift operands of its two instructions, stage 8 runs
exact mod 2^32, and the write-out takes bytes 2..3 with one v_perm_b32 per pair.

No device here.  tests/native/late_scale.cpp drives the injecting P forms and the exact N forms - the plain C++ the header holds beside
the kernel's asm statements, the same expressions - through the butterfly of pass_body, against the unscaled cascade mod 2^32: for
random 32-bit inputs and for 0, +-1, +-2^23, +-2^24, 0x7FFFFFFF, 0x80000000, at every position of a body (both parities of both
stages), for a last pass of three and of two stages, from zero histories and behind a warm-up body, bytes 2..3 must equal
(y >> 9) & 0xFFFF, and the packed pair the words of the reference's write-out in all four formats.  Built with AddressSanitizer and
UBSan, as a program of its own."""
import os
import re
import subprocess

from libacm_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_late_forms_against_the_unscaled_butterfly(tmp_path):
    exe = str(tmp_path / "late_scale")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", _build.CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "late_scale.cpp")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"forms: (\d+) triples\nbodies: (\d+) samples", r.stdout)
    assert m and int(m.group(1)) >= 200000 and int(m.group(2)) >= 4000000, r.stdout[-1000:]


def test_the_kernel_takes_its_forms_from_the_header():
    """the kernel's last pass calls the header's forms and nothing of its own beside them: pass_body names all four, lds_pass hands the
    write-out the description of ITS pass (LastOut<L, G>), and the two-shift path is still there for a last pass of one stage"""
    src = open(os.path.join(_build.CSRC, "acm_kernels.hip")).read()
    body = src[src.index("void pass_body("):src.index("void clear_hist(")]
    for form in ("p_inject_even", "p_inject_odd", "n_exact_sub", "n_exact_add"):
        assert body.count("acm_late::" + form + "(z0, z1, z2)") == 1, form
    assert "using W = LastOut<L, G>;" in src and "pass_body<L, K0, G, LAST && W::LATE>" in src
    assert "PRESHIFT = OutScale<L>::PRESHIFT && !LATE" in src
    hdr = open(os.path.join(_build.CSRC, "acm_late_scale.h")).read()
    assert "ON = (L == 9 && G >= 2)" in hdr
