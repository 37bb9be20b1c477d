"""Host time of plan creation, one library against another (plan creation runs on the thread that feeds the device).

    python profiles/plan_cut_timing.py OUT.json LIB_A LIB_B [rounds]

Two workloads, descriptors only (built once by the driver, no device): (a) bench.py's headline - 1024 streams of level 9, 16 rows x 250
blocks - and (b) the 4000-file corpus of BASELINE.json configs[2], both with their byte-plane form.  The driver starts child processes in
turn - A, B, A, B ... `rounds` times each (default 4) - and every child opens the device and, per workload, creates and destroys
capi.Plan(dev, descs, packed=...) (synchronous upload) 3 times to warm up and 5 times on the clock; where the library exports
acmk_plan_cut_visit it then runs the cutter alone the same way, with a visitor that does nothing, at the device's number of compute
units.  OUT.json gets the raw times and the medians.
"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, TIMED = 3, 5


def prepare(path):
    import numpy as np
    from libacm_amd import capi, workload
    out = {}
    for name, batch in (("headline", workload.build_uniform(1024, 9, 16, 250, channels=1, seed0=0, keep_files=0, threads=16)),
                        ("corpus", workload.build_corpus(4000, shapes=workload.corpus_shapes(4000), seed0=0, keep_files=0, threads=16))):
        mf = capi.mform_streams(batch.idx, batch.descs, threads=16)
        n = len(batch.descs)
        out[name + "_descs"] = np.frombuffer(bytes((capi.StreamDesc * n)(*batch.descs)), dtype=np.uint8)
        out[name + "_packed"] = np.frombuffer(bytes((capi.PackedStream * n)(*mf.streams)), dtype=np.uint8)
        del batch, mf
    np.savez(path, **out)


def child(cache):
    import numpy as np
    from libacm_amd import capi
    L = capi.lib()
    data = np.load(cache)
    res = {"lib": os.environ["ACM_HIP_LIB"]}
    with capi.Device(0) as dev:
        for name in ("headline", "corpus"):
            descs = list((capi.StreamDesc * (data[name + "_descs"].size // C.sizeof(capi.StreamDesc))).from_buffer_copy(data[name + "_descs"].tobytes()))
            packed = list((capi.PackedStream * len(descs)).from_buffer_copy(data[name + "_packed"].tobytes()))
            times = []
            for k in range(WARM + TIMED):
                t0 = time.perf_counter()
                plan = capi.Plan(dev, descs, packed=packed)
                t1 = time.perf_counter()
                if k == 0:
                    st = plan.stats()
                    res[name + "_stats"] = {"tiles": st.tiles, "launches": st.launches, "mform_tiles": st.mform_tiles}
                plan.destroy()
                if k >= WARM:
                    times.append(t1 - t0)
            res[name + "_create_s"] = times
            # the share of capi.Plan itself (building the ctypes arrays from the lists): the same call on ready-made arrays
            arr, pk = (capi.StreamDesc * len(descs))(*descs), (capi.PackedStream * len(descs))(*packed)
            times = []
            for k in range(WARM + TIMED):
                h = C.c_void_p()
                t0 = time.perf_counter()
                rc = L.acmhip_plan_create_packed(dev.h, arr, len(descs), pk, None, 0, 0, C.byref(h))
                t1 = time.perf_counter()
                assert rc == 0
                L.acmhip_plan_destroy(h)
                if k >= WARM:
                    times.append(t1 - t0)
            res[name + "_create_native_s"] = times
            if hasattr(L, "acmk_plan_cut_visit"):
                import torch
                cus = torch.cuda.get_device_properties(0).multi_processor_count
                VISIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_size_t)
                noop = VISIT(lambda *a: None)
                L.acmk_plan_cut_visit.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, VISIT, C.c_void_p]
                times = []
                for k in range(WARM + TIMED):
                    t0 = time.perf_counter()
                    rc = L.acmk_plan_cut_visit(cus, arr, len(descs), pk, None, 0, 0, noop, None)
                    t1 = time.perf_counter()
                    assert rc == 0
                    if k >= WARM:
                        times.append(t1 - t0)
                res[name + "_cut_s"], res["cus"] = times, cus
    print("RESULT " + json.dumps(res))


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    out, libs, rounds = sys.argv[1], sys.argv[2:4], int(sys.argv[4]) if len(sys.argv) > 4 else 4
    cache = out + ".descs.npz"
    prepare(cache)
    runs = []
    for r in range(rounds):
        for tag, lib in zip("AB", libs):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cache], env=dict(os.environ, ACM_HIP_LIB=os.path.abspath(lib)),
                               stdout=subprocess.PIPE, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit("child failed (%d) on %s: nothing more is started" % (p.returncode, lib))
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            res["which"], res["round"] = tag, r
            runs.append(res)
            print(tag, r, {k: round(statistics.median(v) * 1e3, 3) for k, v in res.items() if k.endswith("_s")}, flush=True)
    summary = {}
    for tag in "AB":
        for key in sorted({k for res in runs for k in res if k.endswith("_s")}):
            xs = [x for res in runs if res["which"] == tag for x in res.get(key, [])]
            if xs:
                summary["%s_%s" % (tag, key)] = {"n": len(xs), "median_ms": round(statistics.median(xs) * 1e3, 4), "min_ms": round(min(xs) * 1e3, 4),
                                                 "max_ms": round(max(xs) * 1e3, 4)}
    os.remove(cache)
    with open(out, "w") as f:
        json.dump({"script": "profiles/plan_cut_timing.py", "libs": {"A": libs[0], "B": libs[1]}, "warmup": WARM, "timed_per_child": TIMED,
                   "rounds": rounds, "summary": summary, "cus": runs[-1].get("cus"),
                   "stats_of_the_plans": {k: v for k, v in runs[0].items() if k.endswith("_stats")},
                   "raw_ms_in_order_of_running": {"%s_%s" % (tag, key[:-2] + "_ms"): [round(x * 1e3, 3) for res in runs if res["which"] == tag
                                                                                   for x in res.get(key, [])]
                                                  for tag in "AB" for key in sorted({k for res in runs for k in res if k.endswith("_s")})
                                                  if any(key in res for res in runs if res["which"] == tag)}}, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
