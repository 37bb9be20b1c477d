"""What the block index costs as a by-product of a whole decode (acm_batch_decode_indexed), and what offering it costs everyone else.

Four calls, alternating round by round in one process, each ending synchronised (the batch calls return with their streams drained),
PCM device-resident, 16 host threads:
  a  acm_batch_decode of the parent commit's library (--parent-lib: a libacm_hip.so built from the commit before; skipped without it)
  b  acm_batch_decode of this tree
  c  acm_batch_decode_indexed of this tree
  d  acm_batch_index_files followed by acm_batch_decode of this tree (the way to a decode and an index before)
b against a: the price of the nullable marks pointer, to be held against the spread of a against itself.  c against b: the price of the
index.  c against d: what the by-product saves.

Workloads:
  uniform   1024 level-9 streams of 250 blocks of 16 rows (bench.py's default shape), ACM_BATCH_PARSE_DEVICE
  corpus    the 4000-file corpus (libacm_amd.workload.corpus_shapes), ACM_BATCH_PARSE_HOST

Each workload is a child process under a time limit of its own; a step that fails or runs out of time ends the probe.  Warm-up rounds,
then ROUNDS timed ones: every round's wall clock, median, min, max.  The index of c is compared with that of d, mark by mark.

    python profiles/decode_index_probe.py [--parent-lib PATH] [--out probe_out/decode_index.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THREADS = 16


def generate(shapes):
    from concurrent.futures import ThreadPoolExecutor
    from libacm_amd import synth

    def one(i):
        s = shapes[i]
        return synth.generate(seed=synth.BASE_SEED + i, level=s["level"], rows=s["rows"], nblocks=s["nblocks"], channels=s.get("channels", 1),
                              total_values=s.get("total_values", 0))
    with ThreadPoolExecutor(max_workers=THREADS) as ex:
        return list(ex.map(one, range(len(shapes))))


class Parent:
    """the parent commit's library beside this tree's, in the same process: acm_batch_decode through a device handle of its own"""

    def __init__(self, path):
        from libacm_amd import capi
        vp = C.c_void_p
        self.L = C.CDLL(path)
        self.L.acmhip_device_open.argtypes = [C.c_int, vp, C.POINTER(vp)]
        self.L.acmhip_device_close.argtypes = [vp]
        self.L.acmhip_device_close.restype = None
        self.L.acm_batch_decode.argtypes = [vp, C.POINTER(capi.BatchItem), C.c_size_t, C.POINTER(capi.BatchOpts), C.POINTER(capi.BatchTiming)]
        self.h = vp()
        if self.L.acmhip_device_open(0, None, C.byref(self.h)) != 0:
            raise RuntimeError("the parent library cannot open device 0")

    def close(self):
        self.L.acmhip_device_close(self.h)


def measure(files, parse, args):
    import numpy as np
    from libacm_amd import capi
    L = capi.lib()
    n = len(files)
    bufs, items = capi._batch_items(files)
    words = int(L.acm_batch_pcm_words(items, n, 0))
    res = dict(files=n, file_bytes=int(sum(len(f) for f in files)), pcm_words=words, parse=int(parse))
    parent = Parent(args.parent_lib) if args.parent_lib else None
    with capi.Device(0) as dev:
        d_pcm = dev.malloc(max(words, 1) * 2)
        opts = capi.BatchOpts(0, capi.FMT_S16LE, THREADS, 0, parse, 0, d_pcm, words)
        ix = capi._IndexOut(items, n, 0)
        last = {}

        def call(fn, handle, *more):
            tm = capi.BatchTiming()
            rc = fn(handle, items, n, C.byref(opts), *more, C.byref(tm))
            if rc != 0:
                raise RuntimeError("decode failed: %d" % rc)
            return tm

        def a():
            call(parent.L.acm_batch_decode, parent.h)

        def b():
            last["b"] = call(L.acm_batch_decode, dev.h)

        def c():
            last["c"] = call(L.acm_batch_decode_indexed, dev.h, ix.out)

        def d():
            last["d_index"] = capi.batch_index_files(dev, files, parse=parse, threads=THREADS)[0]
            call(L.acm_batch_decode, dev.h)
        variants = [("a_parent_decode", a)] if parent else []
        variants += [("b_decode", b), ("c_decode_indexed", c), ("d_index_then_decode", d)]
        rounds = {name: [] for name, _ in variants}
        for r in range(args.warmup + args.rounds):
            for name, fn in variants:
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if r >= args.warmup:
                    rounds[name].append(dt * 1e3)
        for name, t in rounds.items():
            res[name] = dict(rounds_ms=[round(x, 3) for x in t], median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
        got = ix.result()
        res["same_marks"] = bool(all(np.array_equal(np.asarray(x), np.asarray(y)) and x.end_status == y.end_status for x, y in zip(got, last["d_index"])))
        res["blocks"] = int(sum(max(0, len(x) - 1) for x in got))
        res["index_bytes"] = int(sum(x.nbytes for x in got))
        for k in ("b", "c"):
            res["%s_parsed" % k] = dict(device=int(last[k].device_parsed), host=int(last[k].host_parsed))
        dev.free(d_pcm)
    if parent:
        parent.close()
    return res


def step_uniform(args):
    from libacm_amd import capi
    files = generate([dict(level=9, rows=16, nblocks=args.blocks)] * args.streams)
    return {"uniform_%d_x_%d_blocks" % (args.streams, args.blocks): measure(files, capi.PARSE_DEVICE, args)}


def step_corpus(args):
    from libacm_amd import capi, workload
    files = generate(workload.corpus_shapes(args.corpus))
    return {"corpus_%d" % args.corpus: measure(files, capi.PARSE_HOST, args)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=250)
    ap.add_argument("--corpus", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default="", help="libacm_hip.so built from the parent commit (variant a)")
    ap.add_argument("--step-seconds", type=int, default=240, help="time limit of each GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "probe_out", "decode_index.json"))
    ap.add_argument("--step", choices=["uniform", "corpus"], help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps({"uniform": step_uniform, "corpus": step_corpus}[args.step](args)))
        return 0
    result = dict(threads=THREADS, rounds=args.rounds, warmup=args.warmup, parent_lib=bool(args.parent_lib))
    for step in ("uniform", "corpus"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--parent-lib", args.parent_lib] + \
              [a for k in ("streams", "blocks", "corpus", "warmup", "rounds") for a in ("--" + k, str(getattr(args, k)))]
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
        print("step %s done" % step, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
