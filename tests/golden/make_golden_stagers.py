#!/usr/bin/env python3
"""Record tests/golden/stagers.json: what the public host stagers of an EARLIER commit hand back for the cases of
tests/test_stagers_golden.py.

The fixture is what a rewrite of the stagers is held to, so it must not come from the code under test.  Record it from a build of the
commit before the change (no GPU needed):

    git worktree add /tmp/parent <commit> && cd /tmp/parent && python -c "from libacm_amd import _build; _build.build_hip()"
    cd <this tree> && ACM_HIP_LIB=/tmp/parent/libacm_amd/lib/libacm_hip.so python tests/golden/make_golden_stagers.py <commit>

What the case list is meant to reach is asserted here, on the recorded library's own output.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_stagers_golden as T  # noqa: E402
from libacm_amd import capi  # noqa: E402

NPATCHES = T.INFO_FIELDS.index("npatches")


def main():
    if len(sys.argv) != 2 or not os.environ.get("ACM_HIP_LIB"):
        sys.exit("usage: ACM_HIP_LIB=<library of the commit to record from> make_golden_stagers.py <that commit>")
    got = T.record()
    # every H1 stream has patches, and the calls say so
    h1 = [i for i in got if ":h1_L" in i and i.split(":")[0] in ("index", "file", "mform", "marks") and "max_blocks=0" not in i]
    assert h1 and all(got[i]["info"][NPATCHES] > 0 for i in h1), "an H1 stream without patches"
    # the byte-plane stager writes its form at every level that has one, whatever the block height
    for level in (7, 8, 9, 11, 12):
        for rows in (1, 2, 3, 16, 17):
            r = got["mform:L%d_r%d:force_chans=0,max_blocks=%d" % (level, rows, T.form_blocks(level, rows))]
            assert r["rc"] == 0 and r["mf_rows"] > 0, ("no form", level, rows)
    # a file that ends early: at least one cut has the byte-plane stager write pairs and then fall back
    cut = [i for i in got if i.startswith("mform:cut_L7[")]
    assert any(got[i]["mf_rows"] == 0 and "pairs" not in got[i]["untouched"] for i in cut), "no cut falls back behind written pairs"
    # a window on the H1 stream whose block in front has patches of its own
    f = T.h1_stream(7)
    front = {int(p.sample) // f.bl for p in capi.stage_file(f.data).patches}
    firsts = {int(i.split("first=")[1].split(",")[0]) for i in got if i.startswith("window:h1_L7:")}
    assert any(first - 1 in front for first in firsts if first >= 1), "no H1 window with patches in the block in front"
    with open(os.path.join(HERE, "stagers.json"), "w") as fh:
        fh.write(json.dumps({"recorded_from": sys.argv[1], "cases": got}, indent=0, sort_keys=True) + "\n")
    print("%d cases" % len(got))


if __name__ == "__main__":
    main()
