"""Float32 output of the synthesis kernels (acmhip_plan_launch_f32) against the int16 launch and against the int16 launch followed by
torch's conversion, on one MI355X.

Workload: N streams x level x rows x blocks, staged by the host parser in the byte-plane form and bound as bench.py binds it (the headline:
1024 x level 9 x 16 rows x 250 blocks).  After a warm-up, three things are timed alternately in one process, step by step, on the
library's own stream (HIP events through torch.cuda.ExternalStream, so the torch conversion queues right behind the launch):
  int16       plan.launch into an int16 tensor
  f32         plan.launch_f32 into a float32 tensor
  int16+conv  plan.launch, then pcm.float().mul_(2 ** -15)            (what a torch user does today: two passes)
  int16+mul   plan.launch, then torch.mul(pcm, 2 ** -15, out=f32)     (the conversion as one pass, for reference)
and in the same run every stream's float output is checked against its int16 output (bits of int16 * 2^-15).
Prints one JSON line per workload (medians and spreads in ms, sample rate, byte counts by design).

Traffic is measured separately (rocprofv3 --pmc FETCH_SIZE WRITE_SIZE in a run of its own, --mode pmc here: a few launches of each).

  python profiles/f32_output_bench.py --level 9 --rows 16 --blocks 250 --streams 1024 --steps 100 --warmup 10
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--level", type=int, default=9)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=250)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--mode", choices=["time", "pmc"], default="time",
                    help="pmc: three launches of each kind and nothing else (for a counter-collection run)")
    a = ap.parse_args()

    import torch
    from libacm_amd import capi, workload

    threads = max(4, min(16, workload.usable_cpus()))
    t0 = time.perf_counter()
    b = workload.build_uniform(a.streams, a.level, a.rows, a.blocks, threads=threads)
    dev = capi.Device(0)
    bufs = b.upload(dev)
    d_idx, d_hdr = bufs[0], bufs[1]
    dev.free(bufs[2])
    mf = capi.mform_streams(b.idx, b.descs, threads=threads)
    mf_ptrs = mf.upload(dev)
    plan = capi.Plan(dev, b.descs, packed=mf.streams)
    plan.bind_mform(*mf_ptrs)
    st = plan.stats()
    t_stage = time.perf_counter() - t0

    i16 = torch.empty(b.pcm_words, dtype=torch.int16, device="cuda")
    f32 = torch.empty(b.pcm_words, dtype=torch.float32, device="cuda")
    conv = torch.empty(b.pcm_words, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ext = torch.cuda.ExternalStream(capi.lib().acmhip_device_stream(dev.h))

    def run(kind):
        if kind == "int16":
            plan.launch(d_idx, d_hdr, i16.data_ptr())
        elif kind == "f32":
            plan.launch_f32(d_idx, d_hdr, f32.data_ptr())
        elif kind == "int16+conv":
            plan.launch(d_idx, d_hdr, i16.data_ptr())
            with torch.cuda.stream(ext):
                i16.float().mul_(2 ** -15)
        else:
            plan.launch(d_idx, d_hdr, i16.data_ptr())
            with torch.cuda.stream(ext):
                torch.mul(i16, 2 ** -15, out=conv)

    kinds = ["int16", "f32", "int16+conv", "int16+mul"]
    if a.mode == "pmc":
        for k in ("int16", "f32"):
            for _ in range(3):
                run(k)
            dev.sync()
        print(json.dumps({"mode": "pmc", "level": a.level, "rows": a.rows, "samples": b.samples}))
        return

    # correctness in the same run: every stream's float samples = its int16 samples * 2^-15, bit for bit; nothing written outside them
    i16.fill_(0x5A5A)
    f32.view(torch.int32).fill_(-1)
    torch.cuda.synchronize()
    run("int16")
    run("f32")
    dev.sync()
    mask = np.zeros(b.pcm_words, bool)
    for d in b.descs:
        mask[d.pcm_off:d.pcm_off + d.n_emit] = True
    inside = torch.from_numpy(mask).cuda()
    want = torch.where(inside, (i16.float() * (2.0 ** -15)).view(torch.int32), torch.full_like(f32.view(torch.int32), -1))
    parity = bool(torch.equal(f32.view(torch.int32), want))
    del want, inside, mask

    for _ in range(a.warmup):
        for k in kinds:
            run(k)
    dev.sync()
    times = {k: [] for k in kinds}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(a.steps):
        for k in kinds:
            ev[0].record(ext)
            run(k)
            ev[1].record(ext)
            ev[1].synchronize()
            times[k].append(ev[0].elapsed_time(ev[1]))
    med = {k: statistics.median(v) for k, v in times.items()}
    n = b.samples
    out = {
        "workload": "%d x level %d x %d rows x %d blocks, byte-plane form" % (a.streams, a.level, a.rows, a.blocks),
        "samples": n, "mform_tiles": st.mform_tiles, "steps": a.steps, "warmup": a.warmup, "stage_s": round(t_stage, 1),
        "parity_f32_eq_int16_scaled": parity,
        "median_ms": {k: round(v, 4) for k, v in med.items()},
        "p10_p90_ms": {k: [round(float(np.percentile(v, 10)), 4), round(float(np.percentile(v, 90)), 4)] for k, v in times.items()},
        "gsamples_per_s": {k: round(n / (v * 1e-3) / 1e9, 2) for k, v in med.items()},
        "f32_over_int16_plus_conv": round(med["f32"] / med["int16+conv"], 3),
        "f32_over_int16_plus_mul": round(med["f32"] / med["int16+mul"], 3),
        "f32_over_int16": round(med["f32"] / med["int16"], 3),
    }
    print(json.dumps(out))
    plan.destroy()
    for p in (d_idx, d_hdr) + tuple(mf_ptrs):
        dev.free(p)


if __name__ == "__main__":
    main()
