"""What the last mile of a crop batch costs: GpuDecoder.crop_batch against crop + the torch assembly a caller had to write before it.

Workload: bench.py's default (1024 level-9 streams of 250 blocks of 16 rows, mono), 1024 and 16 384 windows of 22 050 frames at seeded
random positions (window k crops stream k % 1024), as a float32 [N, 1, T] batch and as an int16 [N, T, 1] one.

  (a) crop_batch                                               - acm_batch_decode_windows_dense: synthesis + one launch of acm_dense_rows
  (b) crop, then a slice copy per window into a zeroed tensor  - N launches
  (c) crop, then ONE gather whose int64 index [N, T] is built on the host and uploaded     (--host-index-max windows at most: 8 bytes
                                                                                             per sample of host memory and PCIe)
  (d) crop, then one gather whose index is a broadcast sum on the device of N offsets built on the host and arange(T)
                                                               - the strongest assembly this probe can write

(b), (c), (d) are the parent commit's way to the same tensor; they run on this tree's crop(), which that commit has unchanged.  The
variants alternate inside one process, WARMUP + REPS rounds, wall clock of the call plus torch.cuda.synchronize(); the tensors of the
last round are compared element for element.  Each GPU step is a child process under a time limit of its own; a step that fails or
runs out of time ends the probe.

  --step kernel (a step of its own, meant to run under `rocprofv3 --kernel-trace --stats -- python profiles/dense_crop_probe.py --step
  kernel ...`): crop_batch alone, REPS calls of each shape, so that the trace holds acm_dense_rows' own durations; it also prints the
  bytes the launch moves (2 per sample read, 2 or 4 written, from the shapes) and the box's copy kernel over the same byte count
  (profiles/ubench/libcopybw.so).  ACM_HIP_LIB=libacm_amd/lib/exp/tuning.so ACM_DENSE_NT=1 runs it with non-temporal stores.

    python profiles/dense_crop_probe.py [--windows 1024,16384] [--out probe_out/dense_crop.json]
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

FRAMES = 22050


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
    # a few windows reach past the end of their stream: the padding is part of what is measured and compared
    return [(k % args.streams, int(rng.integers(0, total - FRAMES + (FRAMES // 4 if k % 64 == 63 else 0))), FRAMES) for k in range(n)]


def stats(t):
    return dict(median_ms=round(statistics.median(t) * 1e3, 3), min_ms=round(min(t) * 1e3, 3), max_ms=round(max(t) * 1e3, 3), reps=len(t))


def step_compare(args, n, f32):
    import numpy as np
    import torch
    from libacm_amd import batch, capi
    files = make_files(args)
    dec = batch.GpuDecoder(0, parse=capi.PARSE_AUTO, dtype=torch.float32 if f32 else torch.int16)
    index = dec.build_index(files)
    wins = windows_for(args, n)
    planar = f32
    shape = (n, 1, FRAMES) if planar else (n, FRAMES, 1)
    out_a = torch.empty(n * FRAMES, dtype=dec.dtype, device="cuda:0")
    flat = torch.empty(capi.batch_window_pcm_words(files, wins), dtype=dec.dtype, device="cuda:0")
    ar = torch.arange(FRAMES, device="cuda:0")
    keep = {}

    def a_crop_batch():
        keep["a"], keep["frames"], keep["st"] = dec.crop_batch(files, wins, FRAMES, channels=1, planar=planar, index=index, out=out_a)
        keep["a_kernel_ms"] = dec.timing.kernel_s * 1e3

    def b_slices():
        pcm, offs, counts, st = dec.crop(files, wins, index, out=flat)
        out = torch.zeros(n, FRAMES, dtype=dec.dtype, device="cuda:0")
        for k in range(n):
            out[k, :counts[k]] = pcm[offs[k]:offs[k] + counts[k]]
        keep["b"] = out.view(shape)
        keep["crop_kernel_ms"] = dec.timing.kernel_s * 1e3

    def c_host_index():
        pcm, offs, counts, st = dec.crop(files, wins, index, out=flat)
        o, c = np.asarray(offs, np.int64)[:, None], np.asarray(counts, np.int64)[:, None]
        t = np.arange(FRAMES, dtype=np.int64)[None, :]
        idx = torch.from_numpy(np.where(t < c, o + t, -1)).to("cuda:0")
        out = torch.where(idx >= 0, pcm[idx.clamp_(min=0)], torch.zeros((), dtype=dec.dtype, device="cuda:0"))
        keep["c"] = out.view(shape)

    def d_device_index():
        pcm, offs, counts, st = dec.crop(files, wins, index, out=flat)
        o = torch.tensor(offs, dtype=torch.int64).to("cuda:0")[:, None]
        c = torch.tensor(counts, dtype=torch.int64).to("cuda:0")[:, None]
        out = torch.where(ar[None, :] < c, pcm[(o + ar[None, :]).clamp_(max=pcm.numel() - 1)], torch.zeros((), dtype=dec.dtype, device="cuda:0"))
        keep["d"] = out.view(shape)

    variants = [("a_crop_batch", a_crop_batch), ("b_crop_then_slice_loop", b_slices), ("d_crop_then_gather_device_index", d_device_index)]
    if n <= args.host_index_max:
        variants.insert(2, ("c_crop_then_gather_host_index", c_host_index))
    times = {name: [] for name, _ in variants}
    for r in range(args.warmup + args.reps):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append(time.perf_counter() - t0)
    res = {name: stats(t) for name, t in times.items()}
    a = keep["a"].cpu().numpy()
    res["tensors_equal"] = {k: bool(np.array_equal(a.view(np.uint8), keep[k].cpu().numpy().view(np.uint8))) for k in ("b", "c", "d") if k in keep}
    base = min((res[name] for name in res if name[0] in "bcd" and name != "tensors_equal"), key=lambda s: s["min_ms"])
    spread = max(s["max_ms"] - s["min_ms"] for name, s in res.items() if name != "tensors_equal")
    # the margin: the best parent way's fastest call against crop_batch's slowest; it has to exceed the min-max spread of the repeated
    # calls - the largest one of any variant of this process (the strict reading), and of the two variants that are compared
    pair = max(base["max_ms"] - base["min_ms"], res["a_crop_batch"]["max_ms"] - res["a_crop_batch"]["min_ms"])
    res["verdict"] = dict(best_parent_way_min_ms=base["min_ms"], crop_batch_max_ms=res["a_crop_batch"]["max_ms"],
                          margin_ms=round(base["min_ms"] - res["a_crop_batch"]["max_ms"], 3), largest_min_max_spread_ms=round(spread, 3),
                          spread_of_the_two_compared_ms=round(pair, 3),
                          crop_batch_wins=bool(base["min_ms"] - res["a_crop_batch"]["max_ms"] > spread),
                          crop_batch_wins_over_the_pair_spread=bool(base["min_ms"] - res["a_crop_batch"]["max_ms"] > pair))
    res["inside_the_call"] = dict(crop_batch_kernel_ms=round(keep["a_kernel_ms"], 4), crop_kernel_ms=round(keep["crop_kernel_ms"], 4),
                                  clipped_windows=int(sum(1 for f in keep["frames"] if f < FRAMES)), ok=all(s == 0 for s in keep["st"]))
    dec.dev.close()
    return {"%d_windows_%s" % (n, "float32_planar" if f32 else "int16_interleaved"): res}


def step_kernel(args):
    import torch
    from libacm_amd import batch, capi
    files = make_files(args)
    out = {"library": os.environ.get("ACM_HIP_LIB", "shipped"), "ACM_DENSE_NT": os.environ.get("ACM_DENSE_NT", "")}
    cb = C.CDLL(os.path.join(ROOT, "profiles", "ubench", "libcopybw.so"))
    cb.acm_copy_ceiling_gbs.restype = C.c_double
    cb.acm_copy_ceiling_gbs.argtypes = [C.c_size_t, C.c_char_p, C.c_size_t]
    for f32 in (True, False):
        dec = batch.GpuDecoder(0, parse=capi.PARSE_AUTO, dtype=torch.float32 if f32 else torch.int16)
        index = dec.build_index(files)
        for n in args.windows:
            wins = windows_for(args, n)
            buf = torch.empty(n * FRAMES, dtype=dec.dtype, device="cuda:0")
            k_ms = []
            for r in range(args.warmup + args.reps):
                b, frames, st = dec.crop_batch(files, wins, FRAMES, channels=1, planar=f32, index=index, out=buf)
                if r >= args.warmup:
                    k_ms.append(dec.timing.kernel_s)
            moved = 2 * sum(frames) + (4 if f32 else 2) * n * FRAMES
            name = C.create_string_buffer(96)
            gbs = cb.acm_copy_ceiling_gbs(moved // 2 // 4096 * 4096, name, 96)
            out["%d_windows_%s" % (n, "float32" if f32 else "int16")] = dict(
                synthesis_plus_gather_events=stats(k_ms), gather_bytes_moved=int(moved), copy_kernel_gbs_same_bytes=round(gbs, 1),
                copy_kernel=name.value.decode(), copy_kernel_ms_same_bytes=round(moved / gbs / 1e6, 4) if gbs > 0 else None)
            del buf
        dec.dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--level", type=int, default=9)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=250)
    ap.add_argument("--windows", type=lambda s: [int(v) for v in s.split(",")], default=[1024, 16384])
    ap.add_argument("--host-index-max", type=int, default=1024, help="variant (c) only up to this many windows")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-seconds", type=int, default=280, help="time limit of each GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "probe_out", "dense_crop.json"))
    ap.add_argument("--step", help="(internal) compare:<windows>:<f32 0|1>, or kernel: run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        if args.step == "kernel":
            res = step_kernel(args)
        else:
            _, n, f32 = args.step.split(":")
            res = step_compare(args, int(n), f32 == "1")
        print("RESULT " + json.dumps(res))
        return 0
    result = dict(workload=dict(streams=args.streams, level=args.level, rows=args.rows, blocks=args.blocks, frames=FRAMES))
    for step in ["compare:%d:%d" % (n, f32) for n in args.windows for f32 in (1, 0)]:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--host-index-max", str(args.host_index_max)] + \
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
