#!/usr/bin/env python3
"""Record tests/golden/window_layout.json: what acm_batch_decode_windows of an EARLIER commit lays out for the cases of
tests/test_window_layout.py.

The fixture is the reference the device-free layout (libacm_amd/csrc/acm_window_layout.cpp) is held to, so it must not come from the
code under test.  Record it from a build of the commit before the split, b26c568, with profiles/window_layout_parent_seam.patch applied
(a dry-run switch inside that commit's decode_windows - its own lines up to the arena fetches, its job loops into plain memory, a return
before the device is touched - behind an export with the signature of acmk_window_layout_visit):

    git worktree add /tmp/parent b26c568 && cd /tmp/parent && git apply <this tree>/profiles/window_layout_parent_seam.patch
    python -c "from libacm_amd import _build; _build.build_hip()"          # the product build, not the tuning one
    cd <this tree> && ACM_HIP_LIB=/tmp/parent/libacm_amd/lib/libacm_hip.so python tests/golden/make_golden_window_layout.py b26c568

Neither the seam build nor the recording needs a GPU.  The case list's coverage conditions are asserted here on the recorded front end's
own output.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_window_layout as T  # noqa: E402


def main():
    if len(sys.argv) != 2 or not os.environ.get("ACM_HIP_LIB"):
        sys.exit("usage: ACM_HIP_LIB=<library of the commit to record from> make_golden_window_layout.py <that commit>")
    L = T._lib()
    cases = T.build_cases()
    results = [T.run_case(L, c) for c in cases]
    missing = [what for what, ok in T.coverage(cases, results).items() if not ok]
    assert not missing, "the case list does not reach: %s" % missing
    head = dict({"recorded_from": sys.argv[1], "recorded_with": "profiles/window_layout_parent_seam.patch, product build (no ACM_TUNING)",
                 "cases": len(cases)}, **T.recording(cases, results))
    with open(os.path.join(HERE, "window_layout.json"), "w") as f:
        f.write(json.dumps(head, indent=1) + "\n")
    print("%d cases, %d refused" % (len(cases), len(head["errors"])))


if __name__ == "__main__":
    main()
