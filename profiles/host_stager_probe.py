"""What the host stagers of a file image cost, this tree against the parent commit's library.  One thread, no device.

Two streams: a clean level-9 stream of 16 rows x 250 blocks (bench.py's stream shape) and the level-7 H1 stream of 16 x 40 (indices
outside the blocks' amplitude range: patches).  Calls, each a loop of REPS calls per timing:
  stage_file        acm_stage_file the way a caller outside the library uses it: without room for patches, and again with room when
                    info.npatches says so
  stage_file_mform  acm_stage_file_mform, and acm_stage_file with room when info.npatches says so
  marks_<stager>    the test hook acmk_stage_marks: the staging entry the batch front ends use (0 int16, 1 byte planes, 2 packed).
                    The parent's makes a second pass for the patches of an H1 stream, this tree's keeps them from the first
The two libraries alternate round by round in one process; per call and library: every round, median, min, max, in microseconds per
call.  The rule for "unchanged": this tree's median is no higher than the parent's median plus the parent's own max - min.

    python profiles/host_stager_probe.py --parent-lib <parent libacm_hip.so> [--out probe_out/host_stager.json]
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


def bind(path):
    from libacm_amd import capi
    vp, sz = C.c_void_p, C.c_size_t
    L = C.CDLL(path)
    L.acm_stage_probe.argtypes = [vp, sz, C.c_int, C.POINTER(capi.StageInfo)]
    L.acm_stage_file.argtypes = [vp, sz, C.c_int, vp, vp, sz, vp, sz, C.POINTER(capi.StageInfo)]
    L.acm_stage_file_mform.argtypes = [vp, sz, C.c_int, vp, vp, sz, C.POINTER(capi.StageInfo), vp, C.c_uint64, vp, C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64)]
    L.acmk_stage_marks.argtypes = [vp, sz, C.c_int, C.c_int, vp, sz, C.POINTER(capi.StageInfo)]
    L.acmhip_mform_bytes.argtypes = [C.c_uint32, C.c_uint64]
    L.acmhip_mform_bytes.restype = C.c_uint64
    L.acmhip_mform_pairs.argtypes = [C.c_uint64]
    L.acmhip_mform_pairs.restype = C.c_uint64
    return L


def calls_for(L, data):
    """{name: a function that makes the call once} for one file image, buffers allocated once"""
    import numpy as np
    from libacm_amd import capi
    a = np.frombuffer(data, dtype=np.uint8)
    info = capi.StageInfo()
    assert L.acm_stage_probe(a.ctypes.data, a.size, 0, C.byref(info)) == 0
    bl = info.rows * info.cols
    need = (info.total_values + bl - 1) // bl
    idx, hdr = np.zeros(need * bl, dtype=np.int16), np.zeros((need, 2), dtype=np.uint32)
    marks = np.zeros(need + 1, dtype=capi.BLOCK_MARK_DT)
    nrows = (need * info.rows) & ~1
    blob = np.zeros(int(L.acmhip_mform_bytes(info.level, nrows)) + 256, dtype=np.uint8)
    pairs = np.zeros(int(L.acmhip_mform_pairs(nrows)) + 32, dtype=np.uint32)
    patches = (capi.Patch * (1 << 20))()
    st = capi.StageInfo()
    rows, nbytes = C.c_uint64(), C.c_uint64()

    def with_room():
        if st.npatches:
            assert st.npatches <= len(patches)
            assert L.acm_stage_file(a.ctypes.data, a.size, 0, idx.ctypes.data, hdr.ctypes.data, need, patches, st.npatches, C.byref(st)) == 0

    def stage_file():
        assert L.acm_stage_file(a.ctypes.data, a.size, 0, idx.ctypes.data, hdr.ctypes.data, need, None, 0, C.byref(st)) == 0
        with_room()

    def stage_file_mform():
        assert L.acm_stage_file_mform(a.ctypes.data, a.size, 0, idx.ctypes.data, hdr.ctypes.data, need, C.byref(st), blob.ctypes.data, 0,
                                      pairs.ctypes.data, C.byref(rows), C.byref(nbytes)) == 0
        with_room()

    def marks_of(stager):
        def fn():
            assert L.acmk_stage_marks(a.ctypes.data, a.size, 0, stager, marks.ctypes.data, need, C.byref(st)) == 0
        return fn
    out = {"stage_file": stage_file, "stage_file_mform": stage_file_mform}
    out.update({"marks_%d" % s: marks_of(s) for s in (0, 1, 2)})
    return out, dict(level=info.level, rows=info.rows, blocks=need, bytes=len(data))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libacm_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "probe_out", "host_stager.json"))
    args = ap.parse_args()
    from libacm_amd import capi, synth
    libs = {"parent": bind(args.parent_lib), "tree": bind(capi.lib_path())}
    streams = {
        "clean_L9_16x250": (synth.generate(seed=synth.BASE_SEED, level=9, rows=16, nblocks=250, total_values=250 * 16 * 512), 4),
        "h1_L7_16x40": (synth.generate(seed=synth.BASE_SEED + 857, level=7, rows=16, nblocks=40, total_values=40 * 16 * 128, allow_out_of_range=1,
                                       pwr_min=0, pwr_max=3), 40),
    }
    result = dict(rounds=args.rounds, warmup=args.warmup, unit="us per call")
    for sname, (data, reps) in streams.items():
        fns = {}
        for lname, L in libs.items():
            fns[lname], shape = calls_for(L, data)
        fns["tree"]["stage_file"]()
        res = dict(shape, reps=reps, npatches=int(capi.stage_file(data).info.npatches))
        for call in fns["tree"]:
            t = {lname: [] for lname in libs}
            for r in range(args.warmup + args.rounds):
                for lname in libs:
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        fns[lname][call]()
                    dt = (time.perf_counter() - t0) / reps * 1e6
                    if r >= args.warmup:
                        t[lname].append(dt)
            res[call] = {lname: dict(rounds=[round(x, 1) for x in v], median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))
                         for lname, v in t.items()}
            p, q = res[call]["parent"], res[call]["tree"]
            res[call]["tree_within_parent_noise"] = bool(q["median"] <= p["median"] + (p["max"] - p["min"]))
            print("%-16s %-17s parent %9.1f (%9.1f .. %9.1f)   tree %9.1f (%9.1f .. %9.1f)   %s" % (
                sname, call, p["median"], p["min"], p["max"], q["median"], q["min"], q["max"],
                "within the parent's noise" if res[call]["tree_within_parent_noise"] else "ABOVE the parent's noise"), flush=True)
        result[sname] = res
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
