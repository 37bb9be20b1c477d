"""What the block index of a batch of files costs: the host parser (batch.build_index, 16 threads - the only way before
acm_batch_index_files), and the same parser on the library's own pool (ACM_BATCH_PARSE_HOST), against the device walk
(acm_batch_index_files, ACM_BATCH_PARSE_DEVICE).

Inputs:
  uniform   bench.py's default shape: 1024 level-9 streams of 250 blocks of 16 rows
  corpus    the 4000-file corpus workload (libacm_amd.workload.corpus_shapes), and its first 16 / 64 / 256 / 512 / 1024 files: where the two
            paths meet is the threshold ACM_BATCH_PARSE_AUTO wants

Each input is a child process under a time limit of its own; a step that fails or runs out of time ends the probe.  Warm-up calls, then
REPS timed calls: median, min, max of the wall clock.  Every device-built index is compared with the host's, mark by mark.

    python profiles/index_probe.py [--out probe_out/index_build.json]
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

THREADS = 16


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return dict(median_ms=statistics.median(t) * 1e3, min_ms=min(t) * 1e3, max_ms=max(t) * 1e3, reps=reps)


def generate(shapes):
    from concurrent.futures import ThreadPoolExecutor
    from libacm_amd import synth

    def one(i):
        s = shapes[i]
        return synth.generate(seed=synth.BASE_SEED + i, level=s["level"], rows=s["rows"], nblocks=s["nblocks"], channels=s.get("channels", 1),
                              total_values=s.get("total_values", 0))
    with ThreadPoolExecutor(max_workers=THREADS) as ex:
        return list(ex.map(one, range(len(shapes))))


def measure(dev, files, args):
    import numpy as np
    from libacm_amd import batch, capi
    last = {}

    def host():
        last["host"] = batch.build_index(files, threads=THREADS)

    def device():
        last["dev"] = capi.batch_index_files(dev, files, parse=capi.PARSE_DEVICE, threads=THREADS)
    res = dict(files=len(files), file_bytes=int(sum(len(f) for f in files)))
    res["host_build_index"] = timed(host, args.warmup, args.reps)
    # the library's own pool without a device handle (what ACM_BATCH_PARSE_AUTO falls back to): build_index minus its Python loop
    res["host_pool"] = timed(lambda: capi.batch_index_files(None, files, parse=capi.PARSE_HOST, threads=THREADS), args.warmup, args.reps)
    res["device_batch_index"] = timed(device, args.warmup, args.reps)
    index, tm = last["dev"]
    res["same_marks"] = bool(all(np.array_equal(np.asarray(a), np.asarray(b)) and a.end_status == b.end_status for a, b in zip(last["host"], index)))
    res["timing"] = dict(stage_ms=tm.stage_s * 1e3, h2d_ms=tm.h2d_s * 1e3, kernel_ms=tm.kernel_s * 1e3, d2h_ms=tm.d2h_s * 1e3, total_ms=tm.total_s * 1e3,
                         blocks=int(tm.blocks), device_indexed=int(tm.device_indexed), host_indexed=int(tm.host_indexed),
                         h2d_bytes=int(tm.h2d_bytes), device_bytes=int(tm.device_bytes), groups=int(tm.groups))
    res["index_bytes"] = int(sum(a.nbytes for a in index))
    # what ACM_BATCH_PARSE_AUTO looks at: the batch in streams of its longest stream's size
    words = [len(a) - 1 for a in index]
    for k, f in enumerate(files):
        rc, info = capi.probe(f)
        words[k] *= info.rows * info.cols if rc == 0 else 0
    res["streams_of_longest"] = sum(words) / max(1, max(words))
    last.pop("dev")
    res["auto"] = dict(timed(lambda: capi.batch_index_files(dev, files, parse=capi.PARSE_AUTO, threads=THREADS), 1, 3),
                       device_indexed=int(capi.batch_index_files(dev, files, parse=capi.PARSE_AUTO, threads=THREADS)[1].device_indexed))
    # the group size: only batches above the smallest budget are cut at all
    if res["file_bytes"] > 128 << 20:
        res["by_group_bytes"] = {}
        for mb in (128, 256, 512, 1024):
            r = timed(lambda: last.__setitem__("g", capi.batch_index_files(dev, files, parse=capi.PARSE_DEVICE, threads=THREADS, max_group_bytes=mb << 20)), 1, 3)
            r.update(groups=int(last["g"][1].groups), device_bytes=int(last["g"][1].device_bytes), kernel_ms=last["g"][1].kernel_s * 1e3,
                     h2d_ms=last["g"][1].h2d_s * 1e3)
            res["by_group_bytes"]["%d_MiB" % mb] = r
    return res


def step_uniform(args):
    from libacm_amd import capi
    files = generate([dict(level=9, rows=16, nblocks=args.blocks)] * args.streams)
    with capi.Device(0) as dev:
        return {"uniform_%d_x_%d_blocks" % (args.streams, args.blocks): measure(dev, files, args)}


def step_corpus(args):
    from libacm_amd import capi, workload
    files = generate(workload.corpus_shapes(args.corpus))
    out = {}
    with capi.Device(0) as dev:
        for n in (16, 64, 256, 512, 1024, args.corpus):
            if n <= args.corpus:
                out["corpus_%d" % n] = measure(dev, files[:n], args)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=250)
    ap.add_argument("--corpus", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-seconds", type=int, default=240, help="time limit of each GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "probe_out", "index_build.json"))
    ap.add_argument("--step", choices=["uniform", "corpus"], help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps({"uniform": step_uniform, "corpus": step_corpus}[args.step](args)))
        return 0
    result = dict(threads=THREADS)
    for step in ("uniform", "corpus"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + \
              [a for k in ("streams", "blocks", "corpus", "warmup", "reps") for a in ("--" + k, str(getattr(args, k)))]
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
