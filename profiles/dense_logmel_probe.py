"""What the logarithm inside the feature kernel costs (profiles/dense_logmel_notes.txt): acm_dense_feat's three builds, the second pass
alone, and crop_features(log=) against crop_features followed by the torch recipe.  One GPU process a step; run each under a time limit.
The linear kernel against the parent commit is dense_feat_probe.py --step kernel, once per library (ACM_HIP_LIB).

  --step kernel   acmk_launch_dense_logmel by itself on ROWS rows of seeded noise in buffers of this script's own, under the
                  512 / 160 / 80 bank at 16 kHz, without ACM_FEAT_LOG_TOP (ln, floor 1e-10: one launch) and with it (the Whisper
                  scale: the reset of the maxima, the feature launch, the second pass), alternating: WARMUP launches, then REPS
                  timings of a launch that ends in a device synchronise (host clock), median, min and max.  Two rows of each are held
                  to the numpy model (tests/dense_logmel.py) over the linear launch's bits.
  --step finish   acmk_launch_feat_log_finish alone over the tensor the step before left, the same way; bytes moved a second.
  --step call     ROWS speech + ROWS noise crops of FRAMES frames out of bench.py's kind of streams into ROWS rows at 10 dB:
                  crop_features(log=LogScale.whisper()) against crop_features and the recipe in torch - clamp, log10, amax, maximum,
                  the affine -, alternating, wall clock of the call plus torch.cuda.synchronize(); and how far the two lie apart.

    python profiles/dense_logmel_probe.py --step kernel|finish|call [--rows 1024] [--frames 16000] [--out probe_out/dense_logmel.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from dense_feat_probe import HOP, N_FFT, N_MELS, RATE, SNR_DB, FeatDesc, stats  # noqa: E402


def setup(args):
    """the device, the launchers, noise rows and the bank's tables in buffers of this script's own"""
    import numpy as np
    from libacm_amd import batch, capi
    L = capi.lib()
    L.acmk_launch_feat_twiddle.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    for f in (L.acmk_launch_dense_feat, L.acmk_launch_dense_logmel):
        f.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(FeatDesc), C.c_void_p, C.c_uint32, C.c_void_p]
    L.acmk_launch_feat_log_finish.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(FeatDesc), C.c_uint32, C.c_void_p]
    dev = capi.Device(0)
    st = L.acmhip_device_stream(dev.h)
    bank = batch.MelBank(RATE, N_FFT, None, HOP, N_MELS)
    T, F = args.frames, bank.frames(args.frames)
    rng = np.random.default_rng(0xFEA7)
    x = (rng.standard_normal((args.rows, T)) * 6000).clip(-32768, 32767).astype(np.int16)
    x[:, T // 2:] //= 64                                                # a quiet half: the clamp to the maximum has work to do
    ptrs = []
    for a in (bank.window, bank.cs, bank.mel_first, bank.mel_count, bank.mel_off, bank.mel_w):
        p = dev.malloc(max(a.nbytes, 16))
        dev.upload(p, a)
        ptrs.append(p)
    d_tw = dev.malloc((N_FFT // 32 + 1) * 2 * (N_FFT // 64) * 2 * 1024)
    d_x, d_out, d_max = dev.malloc(x.nbytes + 128), dev.malloc(args.rows * N_MELS * F * 4), dev.malloc(args.rows * 4)
    dev.upload(d_x, x)
    assert L.acmk_launch_feat_twiddle(ptrs[1], N_FFT, d_tw, st) == 0

    def desc(scale):
        flags, floor_q16, mul_q24, offset_q16, top_q16 = scale.record
        return FeatDesc(N_FFT, HOP, N_MELS, bank.flags, ptrs[0], ptrs[2], ptrs[3], ptrs[4], ptrs[5], d_tw, flags, floor_q16, mul_q24, offset_q16, top_q16, d_max)
    return L, dev, st, x, T, F, d_x, d_out, desc


def timed(dev, launch):
    """seconds of one launch that ends in a device synchronise"""
    dev.sync()
    t0 = time.perf_counter()
    rc = launch()
    dev.sync()
    assert rc == 0, rc
    return time.perf_counter() - t0


def model_rows(lin_bits, scale):
    """tests/dense_logmel.py over the linear launch's bits [rows, B, F] -> the float32 the logmel launch writes"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dense_logmel as G
    s = G.Scale("s", *scale.record)
    bits = lin_bits.astype(np.int64)
    e, m = (bits >> 23) - 127, (bits & 0x7FFFFF) | 0x800000
    Lq = np.where(bits != 0, np.maximum(e * 65536 + G.frac(m.astype(np.uint64))[0].astype(np.int64), s.floor_q16), s.floor_q16)
    if s.top:
        Lq = np.maximum(Lq, Lq.reshape(len(Lq), -1).max(axis=1)[:, None, None] - s.top_q16)
    return (G.scaled(Lq, s).astype(np.float64) / 65536.0).astype(np.float32)


def step_kernel(args, finish_only=False):
    import numpy as np
    from libacm_amd import batch
    L, dev, st, x, T, F, d_x, d_out, desc = setup(args)
    scales = {"log_no_top": batch.LogScale(), "log_top": batch.LogScale.whisper()}
    d = {k: desc(s) for k, s in scales.items()}
    lin = np.zeros((args.rows, N_MELS, F), np.uint32)
    assert L.acmk_launch_dense_feat(d_x, args.rows, T, C.byref(d["log_no_top"]), d_out, 0, st) == 0
    dev.sync()
    dev.download(lin, d_out)
    pick = [0, args.rows - 1]
    res = dict(rows=args.rows, frames=T, feature_frames=F, features_out_bytes=lin.nbytes, rows_checked=len(pick))
    if finish_only:
        # the second pass is not idempotent: L goes in again before every timing, outside the clock
        total, per_row = args.rows * N_MELS * F, N_MELS * F
        Lq = np.full(total, -5 * 65536, np.int32)
        mx = np.full(args.rows, 3 * 65536, np.int32)
        t = []
        for r in range(args.warmup + args.reps):
            dev.upload(d_out, Lq)
            dev.upload(d["log_top"].rowmax, mx)
            t.append(timed(dev, lambda: L.acmk_launch_feat_log_finish(d_out, total, per_row, C.byref(d["log_top"]), 0, st)))
        s = stats(t[args.warmup:])
        s.update(bytes_moved=2 * 4 * total, gbytes_per_s=round(2 * 4 * total / (s["median_ms"] * 1e-3) / 1e9, 1))
        res["finish"] = s
    else:
        t = {k: [] for k in d}
        for r in range(args.warmup + args.reps):
            for k in d:
                t[k].append(timed(dev, lambda: L.acmk_launch_dense_logmel(d_x, args.rows, T, C.byref(d[k]), d_out, 0, st)))
        for k in d:
            assert L.acmk_launch_dense_logmel(d_x, args.rows, T, C.byref(d[k]), d_out, 0, st) == 0
            dev.sync()
            got = np.zeros((args.rows, N_MELS, F), np.float32)
            dev.download(got, d_out)
            assert got[pick].tobytes() == model_rows(lin[pick], scales[k]).tobytes(), k
            res[k] = stats(t[k][args.warmup:])
    dev.close()
    return res


def step_call(args):
    import math
    import numpy as np
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from libacm_amd import batch, capi, synth
    n, T = args.rows, args.frames
    with ThreadPoolExecutor(max_workers=16) as ex:
        files = list(ex.map(lambda i: synth.generate(seed=synth.BASE_SEED + i, level=9, rows=16, nblocks=args.blocks), range(args.streams)))
    dec = batch.GpuDecoder(0, parse=capi.PARSE_AUTO, dtype=torch.float32)
    index = dec.build_index(files)
    rng = np.random.default_rng(22055)
    total = args.blocks * 16 << 9
    wins = [(int(rng.integers(0, args.streams)), int(rng.integers(0, total - T)), T) for k in range(2 * n)]
    rows = [batch.Overlay(k, b=n + k, snr_db=SNR_DB) for k in range(n)]
    bank = batch.MelBank(RATE, N_FFT, None, HOP, N_MELS)
    F = bank.frames(T)
    feat = torch.empty(n * N_MELS * F, dtype=torch.float32, device="cuda:0")
    scale = batch.LogScale.whisper()
    keep, ev = {}, {}

    def one_call():
        keep["one"] = dec.crop_features(files, wins, T, bank, rows=rows, index=index, out=feat, log=scale)[0]
        ev.setdefault("crop_features_log", []).append(dec.timing.kernel_s)

    def torch_way():
        y = dec.crop_features(files, wins, T, bank, rows=rows, index=index, out=feat)[0]
        ev.setdefault("crop_features_then_torch", []).append(dec.timing.kernel_s)
        x = torch.clamp(y, min=1e-10).log10()
        x = torch.maximum(x, x.amax(dim=(1, 2), keepdim=True) - 8.0)
        keep["torch"] = (x + 4.0) / 4.0
    variants = [("crop_features_log", one_call), ("crop_features_then_torch", torch_way)]
    t = {name: [] for name, _ in variants}
    for r in range(args.warmup + args.reps):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
    one_call()
    diff = (keep["one"].double() - keep["torch"].double()).abs()
    res = dict(rows=n, frames=T, feature_frames=F, call_wall={k: stats(v[args.warmup:]) for k, v in t.items()},
               kernel_s_events={k: stats(v[args.warmup:]) for k, v in ev.items()},
               largest_distance_to_torch=float("%.3g" % float(diff.max())),
               derived_bound_without_float32_log_error=float("%.3g" % (0.25 * math.log10(2.0) * 1.02 * 2.0 ** -16 + 2.0 ** -17)))
    dec.dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=["kernel", "finish", "call"])
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=16000)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=250)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "probe_out", "dense_logmel.json"))
    args = ap.parse_args()
    res = step_call(args) if args.step == "call" else step_kernel(args, finish_only=args.step == "finish")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
