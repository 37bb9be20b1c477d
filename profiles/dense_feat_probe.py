"""What mel features inside the crop call cost (profiles/dense_feat_notes.txt): acm_dense_feat alone, and crop_features against
crop_overlay(float32) followed by torch.stft, abs() ** 2 and a mel matmul.  One GPU process; run it under a time limit.

  --step kernel   acmk_launch_feat_twiddle once and acmk_launch_dense_feat by itself on ROWS rows of seeded noise in buffers of this
                  script's own, under the 512 / 160 / 80 bank at 16 kHz: WARMUP launches, then REPS timings of a launch that ends in a
                  device synchronise (host clock; a launch is milliseconds long), median, min and max; its int8 multiply-adds per
                  second two ways - as the contract counts them (rows * F * N * (N + 2) * 4 byte products) and as the kernel issues
                  them (whole tiles of 16 frames and of 16 columns) - against the int8 matrix peak, 2.5e15 multiply-adds a second
                  (twice the bf16 rate of 2.5 PF dense).  Two rows of the last launch are held to the numpy model.
  --step call     ROWS speech + ROWS noise crops of FRAMES frames out of bench.py's kind of streams into ROWS rows at 10 dB, and their
                  features: crop_features, and the torch way - crop_overlay into float32, torch.stft (Hann, center, constant padding),
                  abs() ** 2, a matmul with the float mel matrix - alternating, wall clock of the call plus torch.cuda.synchronize().
                  crop_overlay is byte for byte the parent commit's; with ACM_HIP_LIB naming a library without the features call (the
                  parent commit's) the torch way alone runs.

    python profiles/dense_feat_probe.py --step kernel|call [--rows 1024] [--frames 16000] [--out probe_out/dense_feat.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATE, N_FFT, HOP, N_MELS = 16000, 512, 160, 80
SNR_DB = 10.0
I8_PEAK_MAC_PER_S = 2.5e15


def stats(t):
    return dict(median_ms=round(statistics.median(t) * 1e3, 3), min_ms=round(min(t) * 1e3, 3), max_ms=round(max(t) * 1e3, 3), reps=len(t))


class FeatDesc(C.Structure):
    _fields_ = [("n_fft", C.c_uint32), ("hop", C.c_uint32), ("n_mels", C.c_uint32), ("flags", C.c_uint32), ("window", C.c_void_p),
                ("mel_first", C.c_void_p), ("mel_count", C.c_void_p), ("mel_off", C.c_void_p), ("mel_w", C.c_void_p), ("twiddle", C.c_void_p),
                # acmk_launch_dense_logmel's (dense_logmel_probe.py); acmk_launch_dense_feat reads none of them, an older library has none
                ("log_flags", C.c_uint32), ("floor_q16", C.c_int32), ("mul_q24", C.c_uint32), ("offset_q16", C.c_int32), ("top_q16", C.c_uint32),
                ("rowmax", C.c_void_p)]


def step_kernel(args):
    import numpy as np
    from libacm_amd import batch, capi
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    L = capi.lib()
    L.acmk_launch_feat_twiddle.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.acmk_launch_dense_feat.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(FeatDesc), C.c_void_p, C.c_uint32, C.c_void_p]
    dev = capi.Device(0)
    st = L.acmhip_device_stream(dev.h)
    bank = batch.MelBank(RATE, N_FFT, None, HOP, N_MELS)
    T, F = args.frames, bank.frames(args.frames)
    rng = np.random.default_rng(0xFEA7)
    x = (rng.standard_normal((args.rows, T)) * 6000).clip(-32768, 32767).astype(np.int16)
    tables = [bank.window, bank.cs, bank.mel_first, bank.mel_count, bank.mel_off, bank.mel_w]
    ptrs = []
    for a in tables:
        p = dev.malloc(max(a.nbytes, 16))
        dev.upload(p, a)
        ptrs.append(p)
    nbt, ksteps = N_FFT // 32 + 1, N_FFT // 64
    d_tw = dev.malloc(nbt * 2 * ksteps * 2 * 1024)
    d_x = dev.malloc(x.nbytes + 128)
    d_out = dev.malloc(args.rows * N_MELS * F * 4)
    dev.upload(d_x, x)
    assert L.acmk_launch_feat_twiddle(ptrs[1], N_FFT, d_tw, st) == 0
    desc = FeatDesc(N_FFT, HOP, N_MELS, bank.flags, ptrs[0], ptrs[2], ptrs[3], ptrs[4], ptrs[5], d_tw)
    t = []
    for r in range(args.warmup + args.reps):
        dev.sync()
        t0 = time.perf_counter()
        rc = L.acmk_launch_dense_feat(d_x, args.rows, T, C.byref(desc), d_out, 0, st)
        dev.sync()
        t.append(time.perf_counter() - t0)
        assert rc == 0, rc
    got = np.zeros((args.rows, N_MELS, F), np.float32)
    dev.download(got, d_out)
    import dense_feat as M
    model = M.design("probe", RATE, N_FFT, None, HOP, N_MELS)
    for k in (0, args.rows - 1):
        assert got[k].tobytes() == M.features(x[k], model).tobytes(), k
    s = stats(t[args.warmup:])
    sec = s["median_ms"] * 1e-3
    nominal = args.rows * F * N_FFT * (N_FFT + 2) * 4
    issued = args.rows * -(-F // 16) * 16 * N_FFT * nbt * 32 * 4
    s.update(rows=args.rows, frames=T, feature_frames=F, nominal_i8_macs=nominal, issued_i8_macs=issued, nominal_mac_per_s=float("%.4g" % (nominal / sec)),
             issued_mac_per_s=float("%.4g" % (issued / sec)), i8_peak_mac_per_s=I8_PEAK_MAC_PER_S, nominal_share_of_peak=round(nominal / sec / I8_PEAK_MAC_PER_S, 4),
             issued_share_of_peak=round(issued / sec / I8_PEAK_MAC_PER_S, 4), rows_in_bytes=x.nbytes, features_out_bytes=got.nbytes,
             twiddle_bytes_read_per_workgroup=nbt * 2 * ksteps * 2 * 1024, rows_checked=2)
    for p in ptrs + [d_tw, d_x, d_out]:
        dev.free(p)
    dev.close()
    return s


def step_call(args):
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
    has = hasattr(capi.lib(), "acm_batch_decode_windows_features")
    F = 1 + T // HOP
    wave = torch.empty(n * T, dtype=torch.float32, device="cuda:0")
    feat = torch.empty(n * N_MELS * F, dtype=torch.float32, device="cuda:0")
    hann = torch.hann_window(N_FFT, periodic=True, device="cuda:0")
    # the float mel matrix of the same design (HTK, no normalisation)
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    corner = 700.0 * (10.0 ** (mel(RATE / 2.0) * np.arange(N_MELS + 2) / (N_MELS + 1) / 2595.0) - 1.0)
    fk = np.arange(N_FFT // 2 + 1) * float(RATE) / N_FFT
    W = np.stack([np.maximum(0.0, np.minimum((fk - corner[b]) / (corner[b + 1] - corner[b]), (corner[b + 2] - fk) / (corner[b + 2] - corner[b + 1])))
                  for b in range(N_MELS)])
    Wt = torch.tensor(W, dtype=torch.float32, device="cuda:0")
    keep, ev = {}, {}

    def torch_way():
        x = dec.crop_overlay(files, wins, rows, T, index=index, out=wave)[0]
        ev.setdefault("crop_overlay_stft_mel_torch", []).append(dec.timing.kernel_s)
        spec = torch.stft(x[:, 0], N_FFT, HOP, N_FFT, hann, center=True, pad_mode="constant", return_complex=True)
        keep["torch"] = torch.matmul(Wt, spec.abs() ** 2)
    variants = [("crop_overlay_stft_mel_torch", torch_way)]
    if has:
        bank = batch.MelBank(RATE, N_FFT, None, HOP, N_MELS)

        def one_call():
            keep["feat"] = dec.crop_features(files, wins, T, bank, rows=rows, index=index, out=feat)[0]
            ev.setdefault("crop_features", []).append(dec.timing.kernel_s)
        variants.append(("crop_features", one_call))
    t = {name: [] for name, _ in variants}
    for r in range(args.warmup + args.reps):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
    res = dict(library=os.environ.get("ACM_HIP_LIB", "shipped"), rows=n, frames=T, feature_frames=F, call_wall={k: stats(v[args.warmup:]) for k, v in t.items()},
               kernel_s_events={k: stats(v[args.warmup:]) for k, v in ev.items()})
    if has:
        a, b = keep["feat"].double(), keep["torch"].double() * (32639.0 / 32768.0) ** 2
        live = b > b.amax() * 2.0 ** -40
        res.update(one_call_against_torch_max_rel=float("%.3g" % float(((a - b).abs()[live] / b[live]).max())),
                   one_call_against_torch_median_rel=float("%.3g" % float(((a - b).abs()[live] / b[live]).median())),
                   features_compared=int(live.sum()))
    dec.dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=["kernel", "call"])
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=16000)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=250)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "probe_out", "dense_feat.json"))
    args = ap.parse_args()
    res = step_kernel(args) if args.step == "kernel" else step_call(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
