#!/usr/bin/env python3
"""Record tests/golden/kernel_geo.json: what the acmk_* queries of an EARLIER commit answer over the grid of tests/test_kernel_geo.py.

The fixture is the reference acm_kernel_geo.cpp is held to, so it must not come from the code under test.  Record it from a build of the
commit before the queries left the kernels' translation units - its product library and its tuning library, both built by build_all:

    git worktree add /tmp/parent de0d788 && (cd /tmp/parent && python -c "import __graft_entry__ as g; g.build()")
    cd <this tree> && python tests/golden/make_golden_kernel_geo.py --lib /tmp/parent/libacm_amd/lib de0d788

Each recording is made in a fresh child process that loads the library through ACM_HIP_LIB, the tuning library once per setting of
ACM_K3 / ACM_K2M_G0 (read once per process).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_kernel_geo as T  # noqa: E402


def main():
    if len(sys.argv) != 4 or sys.argv[1] != "--lib":
        sys.exit("usage: make_golden_kernel_geo.py --lib <libacm_amd/lib of the commit to record from> <that commit>")
    paths = {"shipped": os.path.join(sys.argv[2], "libacm_hip.so"), "tuning": os.path.join(sys.argv[2], "exp", "tuning.so")}
    configs = {T.config_name(lib, env): T.record_in_child(os.path.abspath(paths[lib]), env) for lib, env in T.CONFIGS}
    with open(T.GOLDEN, "w") as f:
        f.write('{\n "recorded_from": %s,\n "configs": {\n' % json.dumps(sys.argv[3]))
        f.write(",\n".join('  %s: {\n%s\n  }' % (json.dumps(name), ",\n".join("   %s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":")))
                                                                                 for k, v in rec.items()))
                           for name, rec in configs.items()))
        f.write("\n }\n}\n")
    print("%d configurations, %d bytes" % (len(configs), os.path.getsize(T.GOLDEN)))


if __name__ == "__main__":
    main()
