#!/usr/bin/env python3
"""Record tests/golden/ref_answers.json: the REAL reference's answers to the questions of the tests that compare against it
(tests/test_oracle_vs_ref.py, the seek walks of tests/test_libacm_api.py and the damaged streams of tests/damaged_streams.py,
helpers.RefAnswers).

Runs those tests in this process with the live reference (oracle/_ref, built by `make -C oracle ref`; only where its sources
are), so every answer is an observation of the compiled reference, and the tests pass against it while recording.

  python tests/golden/make_golden_ref_answers.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pytest  # noqa: E402

import helpers  # noqa: E402
import oracle_api as O  # noqa: E402

TESTS = ["tests/test_oracle_vs_ref.py",
         "tests/test_libacm_api.py::test_random_seek_walk_matches_reference",
         "tests/test_libacm_api.py::test_random_seek_walk_pcm",
         "tests/test_libacm_api.py::test_seek_walk_on_a_stale_table_stream",
         "tests/test_damaged_streams.py::test_oracle_matches_the_reference"]


def main():
    if not O.have_ref():
        raise SystemExit("make_golden_ref_answers.py: no compiled reference (oracle/_ref)")
    helpers.RECORDING = {}
    os.chdir(ROOT)
    rc = pytest.main(["-q", "-p", "no:cacheprovider", "-m", "not gpu"] + TESTS)
    if rc != 0:
        raise SystemExit("make_golden_ref_answers.py: the tests failed against the live reference (rc %d)" % rc)
    with open(helpers.REF_ANSWERS, "w") as f:
        json.dump(helpers.RECORDING, f, indent=0, sort_keys=True)
    print("wrote %s: %d tests, %d answers, %d bytes" % (helpers.REF_ANSWERS, len(helpers.RECORDING),
                                                        sum(len(v) for v in helpers.RECORDING.values()),
                                                        os.path.getsize(helpers.REF_ANSWERS)))


if __name__ == "__main__":
    main()
