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

  --mix (profiles/dense_mix_notes.txt): the streams alternate mono and stereo and levels 7, 8, 9 file by file, as workload.corpus_shapes
  does, each with the default workload's sample count; batches of C = 1 and C = 2, float32 [N, C, T] and int16 [N, T, C].
    (a) crop_batch(mix=True)                                   - one call, acm_dense_mixed converts the rows of the other channel count
    (b) two crop_batch calls, one per channel count, the torch conversion of the second one's rows - the integer (L + R) >> 1, or the
        sample into both channels - and an index_copy of both into the batch: the way to the same tensor without ACM_DENSE_MIX
  With --step kernel --mix the trace holds acm_dense_mixed (the mixed batch) and acm_dense_rows (a batch of equal bytes over the files
  of one channel count) side by side.  --parent-lib <the parent commit's libacm_hip.so>: per shape also the batch of one channel count -
  the call that must cost what it cost - on that library and, without and with the flag alternating, on this tree's.

  --rates (profiles/dense_resample_notes.txt): the default workload's streams, a third each at 11025, 22050 and 44100 Hz; one-second
  crops of every file (its own rate in frames) as a float32 [N, 1, 22050] batch.
    rates:<n>:1  crop_batch(rate=22050): acm_dense_resample filters two rows in three
    rates:<n>:0  the call without the flag over the same windows clipped to 22050 frames - a row cannot hold more - on this tree and,
                 with --parent-lib, on the parent commit's library in a process of its own
  With --step kernel --rates the trace holds acm_dense_resample's own durations.

  --speed (profiles/dense_speed_notes.txt): ACM_DENSE_SPEED.
    speedflag:<n>   the --rates call with every speed 1/1 (flag 32 on: the same kernels launch) against the same call without the
                    flag, alternating; with --parent-lib also the call without the flag on the parent commit's library
    speedmix:<n>    the default workload's streams at 22050 Hz into a float32 [N, 1, 16000] batch, one second of output a row: window k
                    is played at (9/10, 1/1, 11/10)[k % 3] - wide c = 51, exact 320 : 441, wide c = 42 - in one call; the three groups
                    as three crop_batch calls plus index_copy; and the rate=-only call of the same shape (every window 22050 frames;
                    with --parent-lib also on the parent's library)
  With --step kernel --speed the trace holds, call after call, batches of ONE speed - 1/1 (acm_dense_resample, K = 24), 9/10
  (acm_dense_speed, K = 22), 11/10 (K = 26) - and the batch of thirds.

  --overlay (profiles/dense_overlay_notes.txt): acm_batch_decode_windows_overlay.  N speech + N noise one-second crops of the default
  workload's streams into N float32 rows at 10 dB.
    overlay:<n>   crop_overlay (one call); crop_overlay of 2N identity rows; crop_batch of the 2N rows; crop_batch + the torch assembly
                  (energies, gain, add, clamp - the noise rows are a slice of the batch, so the assembly pays no gather), alternating.
                  With --parent-lib the last two also on the parent commit's library, a process of its own.  The one call and the
                  torch way are compared within float, not byte for byte.
  With --step kernel --overlay the trace holds the gather launch into the source arena (acm_dense_rows), acm_dense_energy and
  acm_dense_overlay; the step prints the bytes each moves and the box's copy kernel over the same byte counts.

    python profiles/dense_crop_probe.py [--mix | --rates | --speed | --overlay] [--windows 1024,16384] [--out probe_out/dense_crop.json]
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
        if args.mix:
            level = 7 + i % 3
            return synth.generate(seed=synth.BASE_SEED + i, level=level, rows=args.rows, nblocks=args.blocks << (args.level - level), channels=1 + i % 2)
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


def mix_windows(args, n, only=None):
    """(file, first_frame, FRAMES) over the alternating streams (file i has 1 + i % 2 channels); only: files of that channel count"""
    import numpy as np
    rng = np.random.default_rng(22051)
    total = args.blocks * args.rows << args.level
    wins = []
    for k in range(n):
        f = k % args.streams if only is None else (2 * k + only - 1) % args.streams
        frames = total // (1 + f % 2)
        wins.append((f, int(rng.integers(0, frames - FRAMES + (FRAMES // 4 if k % 64 == 63 else 0))), FRAMES))
    return wins


def step_mix(args, n, f32, C):
    import numpy as np
    import torch
    from libacm_amd import batch, capi
    files = make_files(args)
    dec = batch.GpuDecoder(0, parse=capi.PARSE_AUTO, dtype=torch.float32 if f32 else torch.int16)
    index = dec.build_index(files)
    wins = mix_windows(args, n)
    planar = f32
    own = [k for k, w in enumerate(wins) if 1 + w[0] % 2 == C]
    other = [k for k, w in enumerate(wins) if 1 + w[0] % 2 != C]
    i_own, i_other = (torch.tensor(v, dtype=torch.int64, device="cuda:0") for v in (own, other))
    w_own, w_other = [wins[k] for k in own], [wins[k] for k in other]
    out_a = torch.empty(n * C * FRAMES, dtype=dec.dtype, device="cuda:0")
    buf_own = torch.empty(len(own) * C * FRAMES, dtype=dec.dtype, device="cuda:0")
    buf_other = torch.empty(len(other) * (3 - C) * FRAMES, dtype=dec.dtype, device="cuda:0")
    keep = {}

    def a_mix():
        keep["a"], keep["frames"], keep["st"] = dec.crop_batch(files, wins, FRAMES, channels=C, planar=planar, index=index, out=out_a, mix=True)
        keep["a_kernel_ms"] = dec.timing.kernel_s * 1e3

    def b_two_calls():
        x, _, _ = dec.crop_batch(files, w_own, FRAMES, channels=C, planar=planar, index=index, out=buf_own)
        y, _, _ = dec.crop_batch(files, w_other, FRAMES, channels=3 - C, planar=False, index=index, out=buf_other)          # [n, T, 3 - C]
        if C == 1:
            q = (y * 32768.0).to(torch.int32) if f32 else y.to(torch.int32)
            q = (q[:, :, 0] + q[:, :, 1]) >> 1
            y = (q.to(torch.float32) * 2.0 ** -15 if f32 else q.to(torch.int16)).view((len(other), 1, FRAMES) if planar else (len(other), FRAMES, 1))
        else:
            y = y.view(len(other), 1, FRAMES).expand(-1, 2, -1) if planar else y.expand(-1, -1, 2)
        out = torch.empty((n,) + tuple(x.shape[1:]), dtype=dec.dtype, device="cuda:0")
        out.index_copy_(0, i_own, x)
        out.index_copy_(0, i_other, y.contiguous())
        keep["b"] = out

    variants = [("a_crop_batch_mix", a_mix), ("b_two_calls_convert_index_copy", b_two_calls)]
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
    a, b = res["a_crop_batch_mix"], res["b_two_calls_convert_index_copy"]
    res["tensors_equal"] = bool(np.array_equal(keep["a"].cpu().numpy().view(np.uint8), keep["b"].cpu().numpy().view(np.uint8)))
    pair = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    res["verdict"] = dict(two_calls_min_ms=b["min_ms"], mix_max_ms=a["max_ms"], margin_ms=round(b["min_ms"] - a["max_ms"], 3),
                          spread_of_the_two_compared_ms=round(pair, 3), mix_wins=bool(b["min_ms"] - a["max_ms"] > pair))
    res["inside_the_call"] = dict(mix_kernel_ms=round(keep["a_kernel_ms"], 4), converted_rows=len(other),
                                  clipped_windows=int(sum(1 for f in keep["frames"] if f < FRAMES)), ok=all(s == 0 for s in keep["st"]))
    dec.dev.close()
    return {"%d_windows_c%d_%s" % (n, C, "float32_planar" if f32 else "int16_interleaved"): res}


def step_flag(args, n, f32, ch):
    """a batch over the files of ONE channel count - the call that runs acm_dense_rows whatever the flag says - without ACM_DENSE_MIX and,
    where the loaded library knows the flag, with it, alternating; ACM_HIP_LIB names the library (the parent commit's knows no flag)"""
    import torch
    from libacm_amd import batch, capi
    files = make_files(args)
    dec = batch.GpuDecoder(0, parse=capi.PARSE_AUTO, dtype=torch.float32 if f32 else torch.int16)
    index = dec.build_index(files)
    wins = mix_windows(args, n, only=ch)
    buf = torch.empty(n * ch * FRAMES, dtype=dec.dtype, device="cuda:0")
    variants = [("plain", False)]
    try:
        dec.crop_batch(files, wins[:4], FRAMES, channels=ch, planar=f32, index=index, out=buf, mix=True)
        variants.append(("flag", True))
    except Exception:
        pass
    times = {name: [] for name, _ in variants}
    for r in range(args.warmup + args.reps):
        for name, mix in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.crop_batch(files, wins, FRAMES, channels=ch, planar=f32, index=index, out=buf, mix=mix)
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append(time.perf_counter() - t0)
    dec.dev.close()
    return {name: stats(t) for name, t in times.items()}


RATES = (11025, 22050, 44100)


def rate_files(args):
    """the default workload's streams, a third each at 11025, 22050 and 44100 Hz (file i: RATES[i % 3]), mono"""
    from concurrent.futures import ThreadPoolExecutor
    from libacm_amd import synth, workload
    with ThreadPoolExecutor(max_workers=min(16, workload.usable_cpus())) as ex:
        return list(ex.map(lambda i: synth.generate(seed=synth.BASE_SEED + i, level=args.level, rows=args.rows, nblocks=args.blocks,
                                                    rate=RATES[i % 3]), range(args.streams)))


def rate_windows(args, n, clip):
    """one-second crops: (file, first_frame, the file's rate in frames) at seeded positions; clip: FRAMES frames at most, what a call
    without ACM_DENSE_RESAMPLE takes of them"""
    import numpy as np
    rng = np.random.default_rng(22052)
    total = args.blocks * args.rows << args.level
    wins = []
    for k in range(n):
        f = k % args.streams
        sec = RATES[f % 3]
        wins.append((f, int(rng.integers(0, total - sec)), min(sec, FRAMES) if clip else sec))
    return wins


def step_rates(args, n, resample):
    """float32 [N, 1, FRAMES] over rate_files: crop_batch(rate=FRAMES) with resample, else the plain call over the clipped windows (on
    whichever library ACM_HIP_LIB names: the parent commit's knows no other).  Wall clock of the call plus synchronize, and the call's own
    event time (synthesis + the gather launch)"""
    import torch
    from libacm_amd import batch, capi
    files = rate_files(args)
    dec = batch.GpuDecoder(0, parse=capi.PARSE_AUTO, dtype=torch.float32)
    index = dec.build_index(files)
    wins = rate_windows(args, n, clip=not resample)
    buf = torch.empty(n * FRAMES, dtype=dec.dtype, device="cuda:0")
    wall, k_ms = [], []
    for r in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b, frames, st = dec.crop_batch(files, wins, FRAMES, channels=1, planar=True, index=index, out=buf, rate=FRAMES if resample else None)
        torch.cuda.synchronize()
        if r >= args.warmup:
            wall.append(time.perf_counter() - t0)
            k_ms.append(dec.timing.kernel_s)
    dec.dev.close()
    return dict(library=os.environ.get("ACM_HIP_LIB", "shipped"), call_wall=stats(wall), synthesis_plus_gather_events=stats(k_ms),
                source_frames=int(sum(w[2] for w in wins)), frames_delivered=int(sum(frames)), ok=all(s == 0 for s in st),
                samples_synthesised=int(dec.timing.samples), blocks_parsed=int(dec.timing.blocks_parsed))


SPEEDS = ((9, 10), (1, 1), (11, 10))
SPEED_RATE = 16000


def speed_windows(args, n, speeds):
    """one second of output a row: (file, first_frame, source frames of that second at the window's speed), and the speeds"""
    import numpy as np
    from libacm_amd import batch
    rng = np.random.default_rng(22053)
    total = args.blocks * args.rows << args.level
    sp = [speeds[k % len(speeds)] for k in range(n)]
    return [(k % args.streams, int(rng.integers(0, total - 2 * FRAMES)), batch.source_frames(SPEED_RATE, FRAMES, SPEED_RATE, sp[k])) for k in range(n)], sp


def timed(variants, args):
    import torch
    times = {name: [] for name, _ in variants}
    for r in range(args.warmup + args.reps):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append(time.perf_counter() - t0)
    return {name: stats(t) for name, t in times.items()}


def step_speed_flag(args, n):
    """the --rates call without flag 32 and - where the loaded library knows it - with it and every speed 1/1, alternating"""
    import torch
    from libacm_amd import batch, capi
    files = rate_files(args)
    dec = batch.GpuDecoder(0, parse=capi.PARSE_AUTO, dtype=torch.float32)
    index = dec.build_index(files)
    wins = rate_windows(args, n, clip=False)
    buf = torch.empty(n * FRAMES, dtype=dec.dtype, device="cuda:0")
    ev = {"rate_only": [], "speed_all_ones": []}

    def call(name, **kw):
        dec.crop_batch(files, wins, FRAMES, channels=1, planar=True, index=index, out=buf, rate=FRAMES, **kw)
        ev[name].append(dec.timing.kernel_s)
    variants = [("rate_only", lambda: call("rate_only"))]
    if hasattr(capi.lib(), "acm_dense_speed_frames"):
        variants.append(("speed_all_ones", lambda: call("speed_all_ones", speed=[(1, 1)] * n)))
    res = timed(variants, args)
    dec.dev.close()
    return dict(library=os.environ.get("ACM_HIP_LIB", "shipped"), call_wall=res,
                synthesis_plus_gather_events={k: stats(v[args.warmup:]) for k, v in ev.items() if v})


def step_speed_mix(args, n):
    import numpy as np
    import torch
    from libacm_amd import batch, capi
    files = make_files(args)
    dec = batch.GpuDecoder(0, parse=capi.PARSE_AUTO, dtype=torch.float32)
    index = dec.build_index(files)
    T = SPEED_RATE
    plain = [(f, a, FRAMES) for f, a, _ in speed_windows(args, n, SPEEDS)[0]]
    buf = torch.empty(n * T, dtype=dec.dtype, device="cuda:0")
    keep, ev = {}, {"rate_only": [], "one_call_three_speeds": []}

    def rate_only():
        dec.crop_batch(files, plain, T, channels=1, planar=True, index=index, out=buf, rate=T)
        ev["rate_only"].append(dec.timing.kernel_s)
    variants = [("rate_only", rate_only)]
    if hasattr(capi.lib(), "acm_dense_speed_frames"):
        wins, sp = speed_windows(args, n, SPEEDS)
        groups = [[k for k in range(n) if k % 3 == g] for g in range(3)]
        bufs = [torch.empty(len(g) * T, dtype=dec.dtype, device="cuda:0") for g in groups]
        idx = [torch.tensor(g, dtype=torch.int64, device="cuda:0") for g in groups]

        def one_call():
            keep["a"], keep["frames"], keep["st"] = dec.crop_batch(files, wins, T, channels=1, planar=True, index=index, out=buf, rate=T, speed=sp)
            ev["one_call_three_speeds"].append(dec.timing.kernel_s)

        def three_calls():
            out = torch.empty(n, 1, T, dtype=dec.dtype, device="cuda:0")
            for g, b, i in zip(groups, bufs, idx):
                x, _, _ = dec.crop_batch(files, [wins[k] for k in g], T, channels=1, planar=True, index=index, out=b, rate=T, speed=[sp[k] for k in g])
                out.index_copy_(0, i, x)
            keep["b"] = out
        variants += [("one_call_three_speeds", one_call), ("three_calls_index_copy", three_calls)]
    res = dict(library=os.environ.get("ACM_HIP_LIB", "shipped"), call_wall=timed(variants, args),
               synthesis_plus_gather_events={k: stats(v[args.warmup:]) for k, v in ev.items() if v})
    if "a" in keep:
        a, b = res["call_wall"]["one_call_three_speeds"], res["call_wall"]["three_calls_index_copy"]
        pair = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
        res["tensors_equal"] = bool(np.array_equal(keep["a"].cpu().numpy().view(np.uint8), keep["b"].cpu().numpy().view(np.uint8)))
        res["verdict"] = dict(three_calls_min_ms=b["min_ms"], one_call_max_ms=a["max_ms"], margin_ms=round(b["min_ms"] - a["max_ms"], 3),
                              spread_of_the_two_compared_ms=round(pair, 3), one_call_wins=bool(b["min_ms"] - a["max_ms"] > pair))
        res["frames_delivered"] = int(sum(keep["frames"]))
        res["ok"] = all(s == 0 for s in keep["st"])
    dec.dev.close()
    return res


def step_kernel_speed(args):
    """REPS calls per batch of ONE speed and of the thirds: the launches' own durations are the trace's"""
    import torch
    from libacm_amd import batch, capi
    files = make_files(args)
    dec = batch.GpuDecoder(0, parse=capi.PARSE_AUTO, dtype=torch.float32)
    index = dec.build_index(files)
    out = {}
    for n in args.windows:
        buf = torch.empty(n * SPEED_RATE, dtype=dec.dtype, device="cuda:0")
        for name, speeds in (("1_1", SPEEDS[1:2]), ("9_10", SPEEDS[:1]), ("11_10", SPEEDS[2:]), ("thirds", SPEEDS)):
            wins, sp = speed_windows(args, n, speeds)
            k_ms = []
            for r in range(args.warmup + args.reps):
                b, frames, st = dec.crop_batch(files, wins, SPEED_RATE, channels=1, planar=True, index=index, out=buf, rate=SPEED_RATE, speed=sp)
                if r >= args.warmup:
                    k_ms.append(dec.timing.kernel_s)
            out["%d_windows_%s" % (n, name)] = dict(synthesis_plus_gather_events=stats(k_ms), frames_delivered=int(sum(frames)),
                                                    source_frames=int(sum(w[2] for w in wins)), ok=all(s == 0 for s in st))
    dec.dev.close()
    return out


SNR_DB = 10.0


def overlay_windows(args, n):
    """n speech and n noise one-second crops of the default workload's streams: windows [0, n) and [n, 2n)"""
    import numpy as np
    rng = np.random.default_rng(22054)
    total = args.blocks * args.rows << args.level
    return [(int(rng.integers(0, args.streams)), int(rng.integers(0, total - FRAMES)), FRAMES) for k in range(2 * n)]


def step_overlay(args, n):
    """n speech + n noise crops into n float32 rows at 10 dB.  On this tree's library: crop_overlay (one call), crop_overlay of 2n
    identity rows, crop_batch of the 2n rows, and crop_batch + the torch assembly (energies, gain, add, clamp; the noise rows are a
    slice, so no gather is paid), alternating.  On the library ACM_HIP_LIB names where it has no overlay call (the parent commit's):
    crop_batch of the 2n rows, and crop_batch + the torch assembly"""
    import numpy as np
    import torch
    from libacm_amd import batch, capi
    files = make_files(args)
    dec = batch.GpuDecoder(0, parse=capi.PARSE_AUTO, dtype=torch.float32)
    index = dec.build_index(files)
    wins = overlay_windows(args, n)
    buf2 = torch.empty(2 * n * FRAMES, dtype=dec.dtype, device="cuda:0")
    buf1 = torch.empty(n * FRAMES, dtype=dec.dtype, device="cuda:0")
    keep, ev = {}, {}
    ratio = 10.0 ** (SNR_DB / 10)

    def note(name):
        ev.setdefault(name, []).append(dec.timing.kernel_s)

    def dense_2n():
        keep["x"], _, keep["st"] = dec.crop_batch(files, wins, FRAMES, channels=1, planar=True, index=index, out=buf2)
        note("crop_batch_2n")

    def torch_way():
        x, _, _ = dec.crop_batch(files, wins, FRAMES, channels=1, planar=True, index=index, out=buf2)
        note("crop_batch_2n_then_torch")
        a, b = x[:n], x[n:]
        ea, eb = a.square().sum(dim=(1, 2)), b.square().sum(dim=(1, 2))
        g = torch.where(eb > 0, torch.sqrt(ea / (eb * ratio).clamp_(min=1e-30)), torch.zeros_like(ea)).clamp_(max=8.0)
        keep["t"] = torch.addcmul(a, b, g[:, None, None]).clamp_(-1.0, 32767.0 / 32768.0)

    variants = [("crop_batch_2n", dense_2n), ("crop_batch_2n_then_torch", torch_way)]
    if hasattr(capi.lib(), "acm_batch_decode_windows_overlay"):
        rows = [batch.Overlay(k, b=n + k, snr_db=SNR_DB) for k in range(n)]
        ident = [batch.Overlay(k) for k in range(2 * n)]

        def one_call():
            keep["o"], keep["gains"], _, keep["st_o"] = dec.crop_overlay(files, wins, rows, FRAMES, channels=1, planar=True, index=index, out=buf1)
            note("crop_overlay")

        def identity():
            keep["i"], _, _, _ = dec.crop_overlay(files, wins, ident, FRAMES, channels=1, planar=True, index=index, out=buf2)
            note("crop_overlay_identity_2n")
        variants += [("crop_overlay", one_call), ("crop_overlay_identity_2n", identity)]
    res = dict(library=os.environ.get("ACM_HIP_LIB", "shipped"), call_wall=timed(variants, args),
               events={k: stats(v[args.warmup:]) for k, v in ev.items()}, ok=all(s == 0 for s in keep["st"]))
    if "o" in keep:
        a, b = res["call_wall"]["crop_overlay"], res["call_wall"]["crop_batch_2n_then_torch"]
        pair = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
        diff = (keep["o"] - keep["t"]).abs()
        res["one_call_against_torch_same_library"] = dict(
            margin_ms=round(b["min_ms"] - a["max_ms"], 3), spread_of_the_two_compared_ms=round(pair, 3), one_call_wins=bool(b["min_ms"] - a["max_ms"] > pair),
            max_abs_difference_lsb=round(float(diff.max()) * 32768, 3), rows_with_a_gain=int(sum(1 for g in keep["gains"] if g[0])),
            median_gain_q12=int(np.median([g[0] for g in keep["gains"]])))
        dec.crop_batch(files, wins, FRAMES, channels=1, planar=True, index=index, out=buf2)
        x = buf2.clone()
        dec.crop_overlay(files, wins, ident, FRAMES, channels=1, planar=True, index=index, out=buf2)
        res["identity_equals_crop_batch"] = bool(torch.equal(x, buf2))
    dec.dev.close()
    return res


def step_kernel_overlay(args):
    """REPS calls of crop_overlay per shape - n rows at 10 dB over 2n sources - so that the trace holds the launches' own durations:
    the gather launch into the source arena (acm_dense_rows), acm_dense_energy and acm_dense_overlay; beside them the bytes each moves
    (from the shapes) and the box's copy kernel over the same byte counts"""
    import torch
    from libacm_amd import batch, capi
    files = make_files(args)
    cb = C.CDLL(os.path.join(ROOT, "profiles", "ubench", "libcopybw.so"))
    cb.acm_copy_ceiling_gbs.restype = C.c_double
    cb.acm_copy_ceiling_gbs.argtypes = [C.c_size_t, C.c_char_p, C.c_size_t]
    dec = batch.GpuDecoder(0, parse=capi.PARSE_AUTO, dtype=torch.float32)
    index = dec.build_index(files)
    out = {}
    for n in args.windows:
        wins = overlay_windows(args, n)
        rows = [batch.Overlay(k, b=n + k, snr_db=SNR_DB) for k in range(n)]
        buf = torch.empty(n * FRAMES, dtype=dec.dtype, device="cuda:0")
        k_ms = []
        for r in range(args.warmup + args.reps):
            dec.crop_overlay(files, wins, rows, FRAMES, channels=1, planar=True, index=index, out=buf)
            if r >= args.warmup:
                k_ms.append(dec.timing.kernel_s)
        moved = dict(acm_dense_rows=(2 + 2) * 2 * n * FRAMES, acm_dense_energy=2 * 2 * n * FRAMES, acm_dense_overlay=(2 + 2 + 4) * n * FRAMES)
        res = dict(synthesis_through_combine_events=stats(k_ms), calls=args.reps + args.warmup)
        for name, nbytes in moved.items():
            label = C.create_string_buffer(96)
            gbs = cb.acm_copy_ceiling_gbs(nbytes // 2 // 4096 * 4096, label, 96)
            res[name] = dict(bytes_moved=int(nbytes), copy_kernel_gbs_same_bytes=round(gbs, 1),
                             copy_kernel_ms_same_bytes=round(nbytes / gbs / 1e6, 4) if gbs > 0 else None)
        out["%d_rows" % n] = res
        del buf
    dec.dev.close()
    return out


def step_kernel_mix(args):
    """REPS calls per shape of the mixed batch (acm_dense_mixed) and of a batch over the files of one channel count (acm_dense_rows): the
    launch's own durations are the trace's; the call's wall clock and event time are printed here"""
    import torch
    from libacm_amd import batch, capi
    files = make_files(args)
    out = {}
    cb = C.CDLL(os.path.join(ROOT, "profiles", "ubench", "libcopybw.so"))
    cb.acm_copy_ceiling_gbs.restype = C.c_double
    cb.acm_copy_ceiling_gbs.argtypes = [C.c_size_t, C.c_char_p, C.c_size_t]
    for f32 in (True, False):
        dec = batch.GpuDecoder(0, parse=capi.PARSE_AUTO, dtype=torch.float32 if f32 else torch.int16)
        index = dec.build_index(files)
        for n in args.windows:
            for ch in (1, 2):
                buf = torch.empty(n * ch * FRAMES, dtype=dec.dtype, device="cuda:0")
                for what, wins, mix in (("mixed", mix_windows(args, n), True), ("one_count", mix_windows(args, n, only=ch), False)):
                    k_ms, wall = [], []
                    for r in range(args.warmup + args.reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        b, frames, st = dec.crop_batch(files, wins, FRAMES, channels=ch, planar=f32, index=index, out=buf, mix=mix)
                        if r >= args.warmup:
                            wall.append(time.perf_counter() - t0)
                            k_ms.append(dec.timing.kernel_s)
                    read = 2 * sum(fr * (1 + w[0] % 2) for fr, w in zip(frames, wins))
                    moved = read + (4 if f32 else 2) * n * ch * FRAMES
                    name = C.create_string_buffer(96)
                    gbs = cb.acm_copy_ceiling_gbs(moved // 2 // 4096 * 4096, name, 96)
                    out["%d_windows_c%d_%s_%s" % (n, ch, "float32" if f32 else "int16", what)] = dict(
                        call_wall=stats(wall), synthesis_plus_gather_events=stats(k_ms), gather_bytes_moved=int(moved),
                        copy_kernel_gbs_same_bytes=round(gbs, 1), copy_kernel_ms_same_bytes=round(moved / gbs / 1e6, 4) if gbs > 0 else None)
                del buf
        dec.dev.close()
    return out


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
    ap.add_argument("--mix", action="store_true", help="mono and stereo streams in one batch: crop_batch(mix=True) against two calls + torch")
    ap.add_argument("--rates", action="store_true", help="files at 11025, 22050 and 44100 Hz in one 22050 Hz batch: crop_batch(rate=22050), and "
                    "the plain call over the same windows clipped to a row (with --parent-lib also on the parent commit's library)")
    ap.add_argument("--speed", action="store_true", help="ACM_DENSE_SPEED: the flag with every speed 1/1 against the call without it, and a batch of "
                    "three speeds in one call against three calls + index_copy and against the rate=-only call (with --parent-lib also on "
                    "the parent commit's library)")
    ap.add_argument("--overlay", action="store_true", help="acm_batch_decode_windows_overlay: n speech + n noise crops into n rows at 10 dB in one "
                    "call against crop_batch + the torch assembly, and an identity-only call against crop_batch (with --parent-lib the torch "
                    "way and crop_batch also on the parent commit's library)")
    ap.add_argument("--parent-lib", help="with --mix: the parent commit's libacm_hip.so; adds, per shape, a batch of one channel count on that "
                    "library and on this tree's without and with the flag (each library a child process of its own)")
    ap.add_argument("--step", help="(internal) compare:<windows>:<f32 0|1>, mix:<windows>:<f32>:<channels>, or kernel: run one step in this "
                    "process and print its JSON")
    args = ap.parse_args()
    if args.step:
        if args.step == "kernel" and args.overlay:
            res = step_kernel_overlay(args)
        elif args.step.startswith("overlay:"):
            res = step_overlay(args, int(args.step.split(":")[1]))
        elif args.step == "kernel" and args.speed:
            res = step_kernel_speed(args)
        elif args.step.startswith("speedflag:"):
            res = step_speed_flag(args, int(args.step.split(":")[1]))
        elif args.step.startswith("speedmix:"):
            res = step_speed_mix(args, int(args.step.split(":")[1]))
        elif args.step == "kernel" and args.rates:
            res = {"%d_windows" % n: step_rates(args, n, True) for n in args.windows}
        elif args.step == "kernel":
            res = step_kernel_mix(args) if args.mix else step_kernel(args)
        elif args.step.startswith("rates:"):
            _, n, resample = args.step.split(":")
            res = step_rates(args, int(n), resample == "1")
        elif args.step.startswith("flag:"):
            _, n, f32, ch = args.step.split(":")
            res = step_flag(args, int(n), f32 == "1", int(ch))
        elif args.step.startswith("mix:"):
            _, n, f32, ch = args.step.split(":")
            res = step_mix(args, int(n), f32 == "1", int(ch))
        else:
            _, n, f32 = args.step.split(":")
            res = step_compare(args, int(n), f32 == "1")
        print("RESULT " + json.dumps(res))
        return 0
    result = dict(workload=dict(streams=args.streams, level=args.level, rows=args.rows, blocks=args.blocks, frames=FRAMES))
    steps = ["compare:%d:%d" % (n, f32) for n in args.windows for f32 in (1, 0)]
    if args.mix:
        steps = ["mix:%d:%d:%d" % (n, f32, ch) for n in args.windows for f32 in (1, 0) for ch in (1, 2)]
    if args.rates:
        steps = ["rates:%d:%d:tree" % (n, r) for n in args.windows for r in (1, 0)]
        steps += ["rates:%d:0:parent" % n for n in args.windows if args.parent_lib]
    if args.speed:
        steps = ["%s:%d:%s" % (what, n, lib) for n in args.windows for what in ("speedflag", "speedmix") for lib in ("tree", "parent")[:2 if args.parent_lib else 1]]
    if args.overlay:
        steps = ["overlay:%d:%s" % (n, lib) for n in args.windows for lib in ("tree", "parent")[:2 if args.parent_lib else 1]]
    if args.mix and args.parent_lib:
        steps += ["flag:%d:%d:%d:%s" % (n, f32, ch, lib) for n in args.windows for f32 in (1, 0) for ch in (1, 2) for lib in ("parent", "tree")]
    for step in steps:
        env = dict(os.environ)
        if step.endswith(":parent"):
            env["ACM_HIP_LIB"] = os.path.abspath(args.parent_lib)
        key, step = step, step.rsplit(":", 1)[0] if step.startswith(("flag:", "rates:", "speedflag:", "speedmix:", "overlay:")) else step
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--host-index-max", str(args.host_index_max)] + ["--mix"] * args.mix + \
              ["--rates"] * args.rates + ["--speed"] * args.speed + ["--overlay"] * args.overlay + \
              [a for k in ("streams", "level", "rows", "blocks", "warmup", "reps") for a in ("--" + k, str(getattr(args, k)))]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_seconds, env=env)
        except subprocess.TimeoutExpired:
            print("step %s ran out of time: nothing more is started" % step)
            return 1
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print("step %s failed (%d): nothing more is started\n%s" % (step, r.returncode, r.stdout[-3000:]))
            return 1
        got = json.loads(line[-1][7:])
        result.update({"one_count_" + key[5:]: got} if key.startswith("flag:") else {key: got} if key.startswith(("rates:", "speed", "overlay:")) else got)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
