#!/usr/bin/env python3
"""Record tests/golden/plan_cut.json: what the launch planner of an EARLIER commit cuts for the cases of tests/test_plan_cut.py.

The fixture is the reference the device-free cutter (libacm_amd/csrc/acm_plan_cut.cpp) is held to, so it must not come from the code
under test.  Record it from a build of the commit before the split, with profiles/plan_cut_parent_seam.patch applied (a dry-run switch
inside that commit's acmhip_plan_create_packed, behind an export with the signature of acmk_plan_cut_visit):

    git worktree add /tmp/parent 219dea5 && cd /tmp/parent && git apply <this tree>/profiles/plan_cut_parent_seam.patch
    python -c "from libacm_amd import _build; _build.build_hip()"          # the product build, not the tuning one
    cd <this tree> && ACM_HIP_LIB=/tmp/parent/libacm_amd/lib/libacm_hip.so python tests/golden/make_golden_plan_cut.py 219dea5

The case list's coverage conditions are asserted here on the recorded planner's own output.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_plan_cut as T  # noqa: E402


def main():
    if len(sys.argv) != 2 or not os.environ.get("ACM_HIP_LIB"):
        sys.exit("usage: ACM_HIP_LIB=<library of the commit to record from> make_golden_plan_cut.py <that commit>")
    L = T._lib()
    cases = T.build_cases(L)
    results = [T.run_case(L, c) for c in cases]
    missing = [what for what, ok in T.coverage(cases, results).items() if not ok]
    assert not missing, "the case list does not reach: %s" % missing
    rec = T.recording(cases, results)
    fps = rec.pop("case_sha256_16")
    head = dict({"recorded_from": sys.argv[1], "recorded_with": "profiles/plan_cut_parent_seam.patch, product build (no ACM_TUNING)",
                 "cases": len(cases)}, **rec)
    rows = ",\n".join("  " + ", ".join('"%s"' % x for x in fps[k:k + 8]) for k in range(0, len(fps), 8))
    with open(os.path.join(HERE, "plan_cut.json"), "w") as f:
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "case_sha256_16": [\n' + rows + "\n ]\n}\n")
    print("%d cases, %d with tables" % (len(cases), sum(1 for r in results if r["tables"])))


if __name__ == "__main__":
    main()
