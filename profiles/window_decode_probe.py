"""What a one-second crop from each of many files costs: whole-file batch decode + slicing against acm_batch_decode_windows.

Workload: bench.py's default (libacm_amd.workload: 1024 level-9 streams of 250 blocks of 16 rows), one window of 22 050 samples per
stream at a seeded random position, device-resident output.

  (a) acm_batch_decode of the whole files with ACM_BATCH_PARSE_AUTO, then slicing       - what a user does without the index
  (b) acm_batch_decode_windows, ACM_BATCH_PARSE_HOST
  (c) acm_batch_decode_windows, ACM_BATCH_PARSE_DEVICE
  (d) build_index, once
  (b), (c) again with 16 and with 256 windows per call: where DEVICE overtakes HOST (the threshold ACM_BATCH_PARSE_AUTO wants)

Each GPU step is a child process under a time limit of its own; a step that fails or runs out of time ends the probe.  Warm-up calls,
then REPS timed calls: median, min, max of the wall clock of the call (it returns with its stream drained).  The PCM of the timed
window calls is compared with (a)'s slices for the first CHECK streams.

    python profiles/window_decode_probe.py [--streams 1024] [--blocks 250] [--out probe_out/window_decode.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW = 22050
CHECK = 48


def make_files(args):
    from concurrent.futures import ThreadPoolExecutor
    from libacm_amd import synth, workload

    def one(i):
        return synth.generate(seed=synth.BASE_SEED + i, level=args.level, rows=args.rows, nblocks=args.blocks)
    with ThreadPoolExecutor(max_workers=min(16, workload.usable_cpus())) as ex:
        return list(ex.map(one, range(args.streams)))


def windows_for(args, n):
    import numpy as np
    rng = np.random.default_rng(22050)
    total = args.blocks * args.rows << args.level
    return [(i, int(rng.integers(0, total - WINDOW)), WINDOW) for i in range(n)]


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return dict(median_ms=statistics.median(t) * 1e3, min_ms=min(t) * 1e3, max_ms=max(t) * 1e3, reps=reps)


def step_whole(args):
    from libacm_amd import capi
    files = make_files(args)
    cap = capi.batch_pcm_words(files)
    with capi.Device(0) as dev:
        d = dev.malloc(cap * 2)
        last = {}

        def call():
            last["r"] = capi.batch_decode_device(dev, files, d, cap, parse=capi.PARSE_AUTO)
        res = timed(call, args.warmup, args.reps)
        st, words, offs, tm = last["r"]
        res.update(ok=all(s == 0 for s in st), samples=int(sum(words)), device_parsed=int(tm.device_parsed), host_parsed=int(tm.host_parsed),
                   h2d_bytes=int(tm.h2d_bytes))
        dev.free(d)
    return {"a_whole_files_auto": res}


def step_windows(args):
    import numpy as np
    from libacm_amd import batch, capi
    files = make_files(args)
    t0 = time.perf_counter()
    index = batch.build_index(files)
    out = {"d_build_index": dict(seconds=time.perf_counter() - t0, bytes=int(sum(a.nbytes for a in index)))}
    with capi.Device(0) as dev:
        # (a)'s slices for the first CHECK streams
        ncheck = min(CHECK, args.streams)
        cap = capi.batch_pcm_words(files[:ncheck])
        d = dev.malloc(cap * 2)
        st, words, offs, _ = capi.batch_decode_device(dev, files[:ncheck], d, cap, parse=capi.PARSE_AUTO)
        whole = np.zeros(cap, dtype=np.uint16)
        dev.download(whole, d)
        dev.free(d)
        for n in sorted({16, 256, args.streams}):
            if n > args.streams:
                continue
            wins = windows_for(args, n)
            cap = capi.batch_window_pcm_words(files[:n], wins)
            d = dev.malloc(cap * 2)
            for name, parse in (("b_host", capi.PARSE_HOST), ("c_device", capi.PARSE_DEVICE)):
                last = {}

                def call():
                    last["r"] = capi.batch_decode_windows_device(dev, files[:n], index[:n], wins, d, cap, parse=parse)
                res = timed(call, args.warmup, args.reps)
                st, words, offs_w, slots, tm = last["r"]
                got = np.zeros(cap, dtype=np.uint16)
                dev.download(got, d)
                same = all(np.array_equal(got[offs_w[k]:offs_w[k] + WINDOW], whole[offs[f] + a:offs[f] + a + WINDOW])
                           for k, (f, a, c) in enumerate(wins[:ncheck]))
                res.update(ok=all(s == 0 for s in st) and all(w == WINDOW for w in words), pcm_matches_whole_decode=bool(same),
                           blocks_parsed=int(tm.blocks_parsed), device_parsed=int(tm.device_parsed), host_parsed=int(tm.host_parsed),
                           h2d_bytes=int(tm.h2d_bytes), stage_ms=tm.stage_s * 1e3, kernel_ms=tm.kernel_s * 1e3)
                out["%s_%d_windows" % (name, n)] = res
            dev.free(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--level", type=int, default=9)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=250)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-seconds", type=int, default=240, help="time limit of each GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "probe_out", "window_decode.json"))
    ap.add_argument("--step", choices=["whole", "windows"], help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps({"whole": step_whole, "windows": step_windows}[args.step](args)))
        return 0
    result = dict(workload=dict(streams=args.streams, level=args.level, rows=args.rows, blocks=args.blocks, window=WINDOW))
    for step in ("whole", "windows"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + \
              [a for k in ("streams", "level", "rows", "blocks", "warmup", "reps") for a in ("--" + k, str(getattr(args, k)))]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_seconds)
        except subprocess.TimeoutExpired:
            print("step %s ran out of time: nothing more is started" % step)
            return 1
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print("step %s failed (%d): nothing more is started\n%s" % (step, r.returncode, r.stdout[-3000:]))
            return 1
        result.update(json.loads(line[-1][7:]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
