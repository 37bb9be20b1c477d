"""acm_batch_decode end to end, one tree against another: the `end_to_end` legs of bench.py --full.

    python profiles/batch_split_timing.py OUT.json TREE_A TREE_B [rounds] [-- extra bench.py arguments]

TREE_A is the reference (the parent commit, built), TREE_B the tree under test.  The driver runs `python bench.py --gpus 1 --full` in
each tree in turn - A, B, A, B ... `rounds` times each (default 5) - and keeps the `end_to_end` block of every line.  Per leg and tree the
figure is the minimum over all invocations of min(total_s_every_call).  B may exceed A by no more than A's own spread on this box:
(largest - smallest of A's per-invocation minima) / smallest.  h2d_bytes, packed_streams and device_parsed are deterministic and must be
equal.  A failed invocation ends the run: nothing more is started.  Raw lines are appended to OUT.json.raw as they come (a run that had
to be split continues from there: invocations already in the file are not repeated); OUT.json gets the figures, the spread and the verdict.
"""
import json
import os
import socket
import subprocess
import sys

LEGS = ("host_parse", "host_parse_int16_staging", "host_parse_packed_staging", "device_parse", "device_parse_int16_staging",
        "device_parse_pinned_out")
EXACT = ("h2d_bytes", "packed_streams", "device_parsed")


def main():
    argv, extra = sys.argv[1:], []
    if "--" in argv:
        argv, extra = argv[:argv.index("--")], argv[argv.index("--") + 1:]
    out, trees, rounds = argv[0], {"A": os.path.abspath(argv[1]), "B": os.path.abspath(argv[2])}, int(argv[3]) if len(argv) > 3 else 5
    raw, runs = out + ".raw", []
    if os.path.exists(raw):
        with open(raw) as f:
            runs = [json.loads(ln) for ln in f if ln.strip()]
    for r in range(rounds):
        for tag in "AB":
            if any(x["which"] == tag and x["round"] == r for x in runs):
                continue
            try:
                p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--full"] + extra, cwd=trees[tag], stdout=subprocess.PIPE, text=True,
                                   timeout=900)
            except subprocess.TimeoutExpired:
                sys.exit("bench.py ran into its time limit in %s: nothing more is started" % trees[tag])
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not lines or "error" in json.loads(lines[-1]).get("end_to_end", {"error": 1}):
                sys.exit("bench.py failed (%d) in %s: nothing more is started" % (p.returncode, trees[tag]))
            line = json.loads(lines[-1])
            run = {"which": tag, "round": r, "host": socket.gethostname(), "value": line.get("value"), "end_to_end": line["end_to_end"]}
            runs.append(run)
            with open(raw, "a") as f:
                f.write(json.dumps(run) + "\n")
            print(tag, r, {leg: min(run["end_to_end"][leg]["total_s_every_call"]) for leg in LEGS}, flush=True)
    legs = {}
    for leg in LEGS:
        mins = {tag: [min(x["end_to_end"][leg]["total_s_every_call"]) for x in runs if x["which"] == tag] for tag in "AB"}
        a, b = min(mins["A"]), min(mins["B"])
        spread = (max(mins["A"]) - a) / a
        exact = {k: [sorted({x["end_to_end"][leg][k] for x in runs if x["which"] == tag}) for tag in "AB"] for k in EXACT}
        legs[leg] = {"A_per_invocation_min_s": mins["A"], "B_per_invocation_min_s": mins["B"], "A_min_s": a, "B_min_s": b,
                     "A_spread": round(spread, 4), "B_over_A": round(b / a - 1, 4), "within_spread": b <= a * (1 + spread),
                     "exact": {k: {"A": v[0], "B": v[1], "equal": v[0] == v[1] and len(v[0]) == 1} for k, v in exact.items()}}
    with open(out, "w") as f:
        json.dump({"script": "profiles/batch_split_timing.py", "bench_arguments": ["--gpus", "1", "--full"] + extra, "rounds": rounds,
                   "invocations": {tag: sum(x["which"] == tag for x in runs) for tag in "AB"}, "hosts": sorted({x["host"] for x in runs}),
                   "headline_value": {tag: [x["value"] for x in runs if x["which"] == tag] for tag in "AB"}, "legs": legs}, f, indent=1)
        f.write("\n")
    print(json.dumps({leg: {k: v for k, v in d.items() if k in ("A_min_s", "B_min_s", "A_spread", "B_over_A", "within_spread")}
                      for leg, d in legs.items()}, indent=1))


if __name__ == "__main__":
    main()
