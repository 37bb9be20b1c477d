"""What reverberation inside crop_overlay costs (profiles/dense_fir_notes.txt): acm_dense_fir alone, the whole call with and without
`reverb`, and the same batch made with crop_batch and torch.fft.

  --step kernel   acmk_launch_dense_fir by itself on rows of seeded noise in a buffer of this script's own: ROWS x FRAMES frames x
                  {256, 4000, 16000} taps, mono and interleaved stereo.  WARMUP launches, then REPS timings of a launch that ends in a
                  device synchronise (host clock; a launch is milliseconds long), the median; its multiply-adds per second three ways -
                  as the issue counts them (rows * channels * frames * taps), as the kernel issues them (whole tap blocks of the
                  stages it does not skip, from the shapes) and against the packed-dot issue peak 256 CUs * 64 lanes * 2 per clock at
                  --clock-mhz.  The last launch's rows are held to the numpy model on a few rows.
  --step call     N speech + N noise crops of FRAMES frames out of bench.py's kind of streams into N float32 rows at 10 dB:
                  crop_overlay, crop_overlay with responses= but nobody named, crop_overlay(reverb=) with one TAPS-tap response on every
                  speech window, and the torch way - crop_batch of the 2N rows, rfft/irfft convolution of the speech rows with the
                  float response, trim, energies, gain, add, clamp - alternating, wall clock of the call plus torch.cuda.synchronize().
                  With ACM_HIP_LIB naming a library without the call (the parent commit's) crop_overlay alone runs.

    python profiles/dense_fir_probe.py --step kernel|call [--rows 1024] [--frames 16000] [--out probe_out/dense_fir.json]
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

TB, STAGE_BLOCKS, UNIT = 64, 8, 2048
SNR_DB = 10.0


def stats(t):
    return dict(median_ms=round(statistics.median(t) * 1e3, 3), min_ms=round(min(t) * 1e3, 3), max_ms=round(max(t) * 1e3, 3), reps=len(t))


def issued_macs(frames, ntaps, delay):
    """multiply-adds one channel's launch issues: per tile, the whole tap blocks of the stages that reach into [0, frames)"""
    nblk = -(-ntaps // TB)
    lead = delay - (ntaps - 1)
    total = 0
    for j0 in range(0, frames, UNIT):
        for kb0 in range(0, nblk, STAGE_BLOCKS):
            nb = min(STAGE_BLOCKS, nblk - kb0)
            s0 = j0 + lead + kb0 * TB
            if s0 < frames and s0 + UNIT + nb * TB > 0:
                total += nb * TB * UNIT
    return total


def step_kernel(args):
    import numpy as np
    from libacm_amd import capi
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    L = capi.lib()
    L.acmk_launch_dense_fir.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p]
    dev = capi.Device(0)
    st = L.acmhip_device_stream(dev.h)
    rng = np.random.default_rng(0xF12)
    peak = 256 * 64 * 2 * args.clock_mhz * 1e6
    out = dict(clock_mhz_assumed=args.clock_mhz, packed_dot_issue_peak_mac_per_s=peak)
    for channels in (1, 2):
        R = args.frames * channels
        src = (rng.standard_normal((args.rows, R)) * 6000).clip(-32768, 32767).astype(np.int16)
        d_src = dev.malloc((2 * args.rows * R + 64) * 2)
        dev.upload(d_src, src)
        for ntaps in args.taps:
            h = rng.standard_normal(ntaps) * np.exp(-6.0 * np.arange(ntaps) / ntaps)
            q = np.trunc(h * (65535 / np.abs(h).sum())).astype(np.int16)
            delay, shift = ntaps // 16, 13
            nblk = -(-ntaps // TB)
            taps = np.zeros(nblk * TB, np.int16)
            taps[:ntaps] = q[::-1]
            rows = np.zeros((args.rows, 6), dtype=np.int32)
            rows[:, 0] = np.arange(args.rows)
            rows[:, 1] = args.rows + np.arange(args.rows)
            rows[:, 3] = nblk
            rows[:, 4] = delay - (ntaps - 1)
            rows[:, 5] = shift
            d_taps, d_rows = dev.malloc(taps.nbytes), dev.malloc(rows.nbytes)
            dev.upload(d_taps, taps)
            dev.upload(d_rows, rows)
            t = []
            for r in range(args.warmup + args.reps):
                dev.sync()
                t0 = time.perf_counter()
                rc = L.acmk_launch_dense_fir(d_src, d_rows, args.rows, d_taps, args.frames, channels, 0, 0, st)
                dev.sync()
                t.append(time.perf_counter() - t0)
                assert rc == 0, rc
            got = np.zeros((args.rows, R), np.int16)
            dev.download(got, d_src + args.rows * R * 2)
            import dense_fir as DF
            for k in (0, args.rows // 2, args.rows - 1):
                want = DF.filtered(src[k], channels, args.frames, False, (q, delay, shift))[0]
                assert np.array_equal(got[k], want), (channels, ntaps, k)
            s = stats(t[args.warmup:])
            sec = s["median_ms"] * 1e-3
            nominal = args.rows * channels * args.frames * ntaps
            issued = args.rows * channels * issued_macs(args.frames, ntaps, delay)
            s.update(nominal_macs=nominal, issued_macs=issued, nominal_mac_per_s=round(nominal / sec, -9), issued_mac_per_s=round(issued / sec, -9),
                     nominal_share_of_peak=round(nominal / sec / peak, 3), issued_share_of_peak=round(issued / sec / peak, 3), rows_checked=3)
            out["c%d_taps%d" % (channels, ntaps)] = s
            print("c%d taps %5d  %s" % (channels, ntaps, json.dumps(s)), flush=True)
            dev.free(d_taps)
            dev.free(d_rows)
        dev.free(d_src)
    dev.close()
    return out


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
    ntaps = args.taps[0]
    h = rng.standard_normal(ntaps) * np.exp(-6.0 * np.arange(ntaps) / ntaps)
    h /= np.abs(h).max()
    buf1 = torch.empty(n * T, dtype=dec.dtype, device="cuda:0")
    buf2 = torch.empty(2 * n * T, dtype=dec.dtype, device="cuda:0")
    keep, ev = {}, {}
    ratio = 10.0 ** (SNR_DB / 10)
    has = hasattr(capi.lib(), "acm_batch_decode_windows_overlay_fir")

    def dry():
        keep["dry"] = dec.crop_overlay(files, wins, rows, T, index=index, out=buf1)[0]
        ev.setdefault("crop_overlay", []).append(dec.timing.kernel_s)
    variants = [("crop_overlay", dry)]
    if has:
        resp = batch.Response(h)
        hq = torch.tensor(resp.taps.astype(np.float32) / 2.0 ** resp.shift, device="cuda:0")
        d = resp.delay
        nfft = 1 << (T + ntaps - 1).bit_length()
        H = torch.fft.rfft(hq, nfft)

        def idle():
            dec.crop_overlay(files, wins, rows, T, index=index, out=buf1, responses=[resp])
            ev.setdefault("crop_overlay_responses_nobody_names", []).append(dec.timing.kernel_s)

        def wet():
            keep["wet"] = dec.crop_overlay(files, wins, rows, T, index=index, out=buf1, responses=[resp], reverb=[0] * n + [None] * n)[0]
            ev.setdefault("crop_overlay_reverb", []).append(dec.timing.kernel_s)

        def torch_way():
            x = dec.crop_batch(files, wins, T, index=index, out=buf2)[0]
            a = torch.fft.irfft(torch.fft.rfft(x[:n, 0], nfft) * H, nfft)[:, d:d + T]
            a = (a * 32768).round_().clamp_(-32768, 32767).div_(32768)[:, None, :]
            b = x[n:]
            ea, eb = a.square().sum(dim=(1, 2)), b.square().sum(dim=(1, 2))
            g = torch.where(eb > 0, torch.sqrt(ea / (eb * ratio).clamp_(min=1e-30)), torch.zeros_like(ea)).clamp_(max=8.0)
            keep["torch"] = torch.addcmul(a, b, g[:, None, None]).clamp_(-1.0, 32767.0 / 32768.0)
        variants += [("crop_overlay_responses_nobody_names", idle), ("crop_overlay_reverb", wet), ("crop_batch_fft_torch", torch_way)]
    t = {name: [] for name, _ in variants}
    for r in range(args.warmup + args.reps):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
    res = dict(library=os.environ.get("ACM_HIP_LIB", "shipped"), rows=n, frames=T, taps=ntaps, call_wall={k: stats(v[args.warmup:]) for k, v in t.items()},
               kernel_s_events={k: stats(v[args.warmup:]) for k, v in ev.items()})
    if has:
        diff = (keep["wet"] - keep["torch"]).abs()              # the last round's: wet ran after dry into the same buffer
        res.update(shift=resp.shift, delay=resp.delay, one_call_against_torch_max_abs_lsb=round(float(diff.max()) * 32768, 2),
                   one_call_against_torch_mean_abs_lsb=round(float(diff.mean()) * 32768, 4))
        wet_rows = keep["wet"].clone()
        dry()
        res["rows_reverb_changes"] = int((wet_rows != keep["dry"]).flatten(1).any(dim=1).sum())
    dec.dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=["kernel", "call"])
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=16000)
    ap.add_argument("--taps", type=lambda s: [int(v) for v in s.split(",")], default=[256, 4000, 16000], help="--step call takes the first")
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=250)
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="the engine clock the share of peak is stated against")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "probe_out", "dense_fir.json"))
    args = ap.parse_args()
    res = step_kernel(args) if args.step == "kernel" else step_call(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
