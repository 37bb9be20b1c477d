"""Float32 PCM (include/acm_hip.h: acmhip_plan_launch_f32, acmhip_host_synth_f32, ACM_BATCH_PCM_F32) without a GPU.

A float sample is EXACTLY the ACMHIP_FMT_S16LE sample times 2^-15 - the reference's own 16-bit value with its wrap, divided by 32768 -
so parity is an equality on bits: out.view(uint32) == (oracle_s16.astype(float32) / 32768).view(uint32).  Here: the host synthesis
(the CPU reference of the float output), the argument checks that need no device, the generated code of the float builds of the lean
kernels (cross-compiled, checked as tests/test_isa_invariants.py checks the int16 builds, with twice the stores) and decode_sharded
with a float32 decoder over two gloo ranks."""
import ctypes as C
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import make_stream, oracle_pcm
from libacm_amd import _build, batch, capi
from test_isa_invariants import basic_blocks, reads_of, regs_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32_bits(s16):
    """the float32 samples of int16 ones (any integer view of them), as uint32 bits"""
    return (np.asarray(s16).view(np.int16).astype(np.float32) / np.float32(32768)).view(np.uint32)


def host_synth_f32(staged, row_begin=0, n_emit=None, patches=True):
    info = staged.info
    cols = 1 << info.level
    nrows = info.blocks * info.rows
    if n_emit is None:
        n_emit = min(info.total_values, nrows * cols) - row_begin * cols
    d = capi.StreamDesc(idx_off=0, hdr_off=0, pcm_off=0, n_emit=n_emit, level=info.level, rows=info.rows, nrows=nrows, row_begin=row_begin)
    out = np.full(n_emit + 8, 0xFFFFFFFF, dtype=np.uint32)
    pl = list(staged.patches) if (patches and staged.patches is not None) else []
    arr = (capi.Patch * max(1, len(pl)))(*pl)
    rc = capi.lib().acmhip_host_synth_f32(C.byref(d), staged.idx.ctypes.data, staged.hdr.ctypes.data, arr if pl else None, len(pl), out.ctypes.data)
    assert rc == 0, rc
    assert (out[n_emit:] == 0xFFFFFFFF).all()           # nothing written behind the last sample asked for
    return out[:n_emit]


@pytest.mark.parametrize("level", list(range(16)))
def test_host_synth_f32_every_level_and_block_height(level):
    """levels 0-15 x block heights 1, 3, 16, 64 (ragged ends, full-range row values: samples that wrap): the s16le samples / 32768, in bits"""
    for rows in (1, 3, 16, 64):
        nb = max(2, min(24, (1 << 15) // (rows << level)))
        if (rows << level) * nb > (1 << 19):
            nb = 1 + ((1 << 19) >> level) // rows
        f = make_stream(7000 + 17 * level + rows, level, rows, nb, cut=7 if level else 1, val_max=65535, pwr_max=15)
        s = capi.stage_file(f)
        want, _ = oracle_pcm(f)
        got = host_synth_f32(s)
        assert got.size == want.size and np.array_equal(got, f32_bits(want)), (level, rows)
        v = got.view(np.float32)
        assert (v >= -1.0).all() and (v < 1.0).all()


def test_host_synth_f32_windows():
    """windows from row 0 and from later rows (the two rows in front are all a window needs) equal the same samples of the whole decode"""
    for lv, rows, nb in ((7, 16, 9), (5, 1, 200), (10, 3, 6), (3, 64, 5), (13, 1, 6)):
        f = make_stream(7300 + lv, lv, rows, nb)
        s = capi.stage_file(f)
        want = f32_bits(oracle_pcm(f)[0])
        cols = 1 << lv
        total_rows = nb * rows
        for rb in (0, 1, 2, 3, rows + 1, total_rows // 2, total_rows - 1):
            n = min(want.size - rb * cols, 5 * cols + 3)
            assert np.array_equal(host_synth_f32(s, row_begin=rb, n_emit=n), want[rb * cols: rb * cols + n]), (lv, rows, rb)


def test_host_synth_f32_h1_patches():
    """hazard H1 streams: the patches apply to the float output as to the int16 one (and without them it differs)"""
    seen = 0
    for seed in range(12):
        f = make_stream(7400 + seed, 6, 8, 30, pwr_min=0, pwr_max=3, mix=1)
        s = capi.stage_file(f)
        if s.patches is None or len(s.patches) == 0:
            continue
        seen += 1
        want = f32_bits(oracle_pcm(f)[0])
        assert np.array_equal(host_synth_f32(s), want)
        assert not np.array_equal(host_synth_f32(s, patches=False), want)
    assert seen >= 3


def test_host_synth_f32_argument_checks():
    L = capi.lib()
    f = make_stream(7500, 5, 4, 6)
    s = capi.stage_file(f)
    d = capi.StreamDesc(idx_off=0, hdr_off=0, pcm_off=0, n_emit=5 * 4 * 32 + 1, level=5, rows=4, nrows=5 * 4, row_begin=0)
    out = np.zeros(2048, dtype=np.float32)
    assert L.acmhip_host_synth_f32(C.byref(d), s.idx.ctypes.data, s.hdr.ctypes.data, None, 0, out.ctypes.data) == capi.ERR_ARG    # past the staged rows
    d.n_emit = 64
    assert L.acmhip_host_synth_f32(C.byref(d), s.idx.ctypes.data, s.hdr.ctypes.data, None, 0, None) == capi.ERR_ARG              # no output
    assert L.acmhip_host_synth_f32(None, s.idx.ctypes.data, s.hdr.ctypes.data, None, 0, out.ctypes.data) == capi.ERR_ARG
    d.level = 16
    assert L.acmhip_host_synth_f32(C.byref(d), s.idx.ctypes.data, s.hdr.ctypes.data, None, 0, out.ctypes.data) == capi.ERR_ARG
    d.level = 5
    assert L.acmhip_host_synth_f32(C.byref(d), s.idx.ctypes.data, s.hdr.ctypes.data, None, 0, out.ctypes.data) == 0
    assert L.acmhip_plan_launch_f32(None, None, None, None) == capi.ERR_ARG


def test_batch_f32_refuses_what_it_cannot_do_before_any_device_work():
    """ACM_BATCH_PCM_F32 without device-resident output, with another format, with the packed staging: ACMHIP_ERR_ARG (checked before the
    device handle is looked at, so a dangling one is enough here)"""
    L = capi.lib()
    f = make_stream(7600, 7, 16, 4)
    bufs, items = capi._batch_items([f])
    dummy = C.c_void_p(1)
    for fmt, flags, d_pcm in ((capi.FMT_S16LE, capi.BATCH_PCM_F32, None),
                              (capi.FMT_S16BE, capi.BATCH_PCM_F32, dummy),
                              (capi.FMT_U16LE, capi.BATCH_PCM_F32, dummy),
                              (capi.FMT_S16LE, capi.BATCH_PCM_F32 | capi.BATCH_STAGE_PACKED, dummy)):
        opts = capi.BatchOpts(0, fmt, 1, 0, capi.PARSE_HOST, flags, d_pcm, 1 << 20)
        assert L.acm_batch_decode(dummy, items, 1, C.byref(opts), None) == capi.ERR_ARG, (fmt, flags)


# ---- generated code of the float builds (acm_kernels_f32.hip) -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def f32_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa_f32") / "acm_kernels_f32.s"
    cmd = [_build.HIPCC, "-O3", "-std=c++17", "--offload-arch=" + _build.GFX, "-I", _build.INC, "-I", _build.CSRC,
           "--cuda-device-only", "-S", "-o", str(out), os.path.join(_build.CSRC, "acm_kernels_f32.hip")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return out.read_text()


def functions(asm):
    kernels = set(re.findall(r"\.type\s+(\S+),@function", asm))
    for m in re.finditer(r"^(_Z\S+):", asm, re.M):
        if m.group(1) in kernels:
            end = asm.index(".Lfunc_end", m.end())
            yield m.group(1), asm[m.end():end].split("\n")


def f32_lean_bodies(asm):
    """the float builds of acm_tile2 and acm_chunk (named outside the int16 scan of tests/test_isa_invariants.py)"""
    for name, lines in functions(asm):
        if re.search(r"acm_f32_(tile2|chunk)", name):
            yield name, lines


def test_float_builds_stay_out_of_the_int16_scan_and_cover_every_lean_kernel(f32_asm):
    names = [n for n, _ in functions(f32_asm)]
    assert not [n for n in names if "acm_tile2" in n or "acm_chunk" in n], "a float build under a name the int16 checks scan"
    tile2 = [n for n in names if "acm_f32_tile2" in n]
    chunk = [n for n in names if "acm_f32_chunk" in n]
    assert len(tile2) >= 19 and len(chunk) == 5, (len(tile2), len(chunk))   # nine levels + the matrix builds of 7-14 (two depths at 13, 14); levels 8-12
    # every other family has its float build too, and the packed form has none
    for k in ("acm_fused_tile_f32", "acm_small_level_f32", "acm_sw_emit_f32"):
        assert any(k in n for n in names), k
    assert not any("acm_tile2p" in n for n in names)
    # the int16 translation unit keeps its kernels and nothing of the float ones
    src = open(os.path.join(_build.CSRC, "acm_kernels_f32.hip")).read()
    assert "#define ACM_OUT_F32 1" in src


def after_first_hand_load(lines):
    """the instructions the control flow reaches from the first hand-issued load on (basic_blocks of tests/test_isa_invariants.py)"""
    first_hand = next(k for k, l in enumerate(lines) if l.strip().startswith(";;#ASMSTART") and lines[k + 1].strip().startswith("global_load"))
    blocks = basic_blocks(lines)
    start = next(k for k, b in enumerate(blocks) if any(ins[0] > first_hand for ins in b[1]))
    seen, work, out = {start}, [start], []
    while work:
        k = work.pop()
        out += [ins for ins in blocks[k][1] if k != start or ins[0] > first_hand]
        for t in blocks[k][2]:
            if t not in seen:
                seen.add(t)
                work.append(t)
    return out


def test_float_builds_read_no_loading_register_before_the_wait(f32_asm):
    """tests/test_isa_invariants.py::test_no_read_of_a_loading_register_before_the_wait over the float builds"""
    n_kernels = 0
    for name, lines in f32_lean_bodies(f32_asm):
        n_kernels += 1
        blocks = basic_blocks(lines)
        state_in = [set() for _ in blocks]
        work = list(range(len(blocks)))
        n_loads = sum(1 for b in blocks for ins in b[1] if ins[1].startswith("global_load"))
        while work:
            k = work.pop()
            pending = set(state_in[k])
            for ln, op, ops, text in blocks[k][1]:
                if op == "s_waitcnt" and "vmcnt" in text:
                    pending = set()
                    continue
                bad = reads_of(op, ops, text) & pending
                assert not bad, "%s line %d reads v%s while its load is in flight: %s" % (name[:60], ln, sorted(bad), text)
                if not op.startswith(("global_store", "ds_write", "s_", "buffer_store")) and ops:
                    clobbered = regs_of(ops[0]) & pending
                    assert not clobbered, "%s line %d writes v%s while a load into it is in flight: %s" % (name[:60], ln, sorted(clobbered), text)
                if op.startswith("global_load"):
                    pending |= regs_of(ops[0])
            for t in blocks[k][2]:
                if not pending <= state_in[t]:
                    state_in[t] |= pending
                    work.append(t)
        assert n_loads >= (12 if "acm_f32_chunk" in name or "Lb1ELi6E" in name else 2 * 9), (name, n_loads)
    assert n_kernels >= 24


def test_float_builds_wait_by_hand_for_twice_the_stores(f32_asm):
    """two vmcnt waits per kernel, vmcnt(0) and vmcnt(#stores), with 8 or 16 dwordx4 stores (twice the int16 build's), non-temporal"""
    n = 0
    for name, lines in f32_lean_bodies(f32_asm):
        n += 1
        assert not any(l.strip().startswith("scratch_") for l in lines), name[:60]
        stores = [l.strip() for l in lines if l.strip().startswith("global_store")]
        assert len(stores) in (8, 16), (name[:60], len(stores))
        assert all(s.startswith("global_store_dwordx4") and s.split(";")[0].rstrip().endswith(" nt") for s in stores), (name[:60], stores[:2])
        if ("Lb1E" in name and "acm_f32_tile2I" in name) or "acm_f32_chunk" in name:
            # the matrix-core builds fill their coefficient tables first, with compiler-tracked loads and waits; in the float builds the
            # compiler lays those blocks out behind the first hand-issued load (they run before it: it branches back), so what counts
            # is what the control flow reaches from that load on
            waits = [ins[3] for ins in after_first_hand_load(lines) if ins[1] == "s_waitcnt" and "vmcnt" in ins[3]]
        else:
            waits = [l.strip() for l in lines if "vmcnt" in l]
        assert sorted(waits) == ["s_waitcnt vmcnt(0)", "s_waitcnt vmcnt(%d)" % len(stores)], (name[:60], waits)
    assert n >= 24


def test_float_builds_keep_phase_priorities_and_chunk_tables(f32_asm):
    """test_phase_priorities_are_in_the_tile_loop and test_chunk_kernel_keeps_its_tables_in_lds over the float builds"""
    for name, lines in f32_lean_bodies(f32_asm):
        prios = [l.split()[1] for l in lines if l.strip().startswith("s_setprio")]
        if "TileCfgILi13ELi1024E" in name or "TileCfgILi14ELi1024E" in name:
            assert prios == [], (name[:60], prios)
        else:
            assert set(prios) == {"0", "2", "3"}, (name[:60], prios)
        if "acm_f32_chunk" in name:
            text = "\n".join(l.split(";")[0] for l in lines)
            assert "flat_" not in text and "scratch_" not in text and "buffer_load" not in text, name[:60]
            assert text.count("s_barrier") == 1, name[:60]
            assert text.count("v_mfma_i32_16x16x64_i8") >= 18 and "v_mul_lo_u32" not in text, name[:60]


def test_float_write_out_converts_with_sdwa_and_packed_multiplies(f32_asm):
    """the widening is v_cvt_f32_i32 with SDWA WORD_0 / WORD_1 (sign-extending) and one v_pk_mul_f32 per pair: 1.5 VALU per sample"""
    for name, lines in f32_lean_bodies(f32_asm):
        text = "\n".join(l.split(";")[0] for l in lines)
        stores = text.count("global_store_dwordx4")
        cvt = len(re.findall(r"v_cvt_f32_i32_sdwa \S+, sext\(\S+\) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_[01]", text))
        pk = text.count("v_pk_mul_f32")
        assert cvt == 4 * stores and pk == 2 * stores, (name[:60], stores, cvt, pk)


# ---- decode_sharded with a float32 decoder ----------------------------------------------------------------------------------------------

def corpus():
    files = []
    for i in range(11):
        lv = [5, 7, 9, 3, 0][i % 5]
        files.append(make_stream(7700 + i, lv, [16, 3, 1][i % 3], 1 + (i * 5) % 7, channels=1 + i % 2, cut=i % 3))
    files.insert(3, b"not an acm file")
    return files


class F32OracleDecoder:
    """GpuDecoder(dtype=torch.float32)'s shape, on the host: the float32 samples of the CPU oracle, streams padded to 64 samples"""
    dtype = torch.float32

    def __call__(self, files, out=None):
        import oracle_api as O
        parts, offsets, words, statuses, pos = [], [], [], [], 0
        for f in files:
            o = O.Oracle(f)
            if o.err < 0:
                offsets.append(0), words.append(0), statuses.append(o.err)
                continue
            o.close()
            pcm, st = O.Oracle.decode_all(f)
            v = f32_bits(pcm).view(np.float32)
            pad = (-v.size) % 64
            parts.append(np.concatenate([v, np.zeros(pad, np.float32)]))
            offsets.append(pos), words.append(v.size), statuses.append(st)
            pos += v.size + pad
        flat = torch.from_numpy(np.concatenate(parts)) if parts else torch.zeros(0, dtype=torch.float32)
        return flat, offsets, words, statuses


def check_f32(out, files):
    for f, (st, pcm) in zip(files, out):
        import oracle_api as O
        o = O.Oracle(f)
        if o.err < 0:
            assert st == o.err and pcm.size == 0
            continue
        o.close()
        want, wst = O.Oracle.decode_all(f)
        assert st == wst and pcm.dtype == np.float32 and np.array_equal(pcm.view(np.uint32), f32_bits(want))


def _worker_f32(rank, world, port, q, chunks):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        files = corpus()
        out = batch.decode_sharded(files, F32OracleDecoder(), dist=dist, root=0, device=torch.device("cpu"), chunks=chunks, ring=2)
        if rank == 0:
            single = batch.decode_sharded(files, F32OracleDecoder())
            assert all(a[0] == b[0] and a[1].dtype == b[1].dtype == np.float32 and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
                       for a, b in zip(out, single))
            check_f32(out, files)
            q.put("ok")
        else:
            assert out is None
    except Exception as e:
        q.put("rank %d: %r" % (rank, e))
    finally:
        dist.destroy_process_group()


def test_single_process_front_end_f32():
    files = corpus()
    check_f32(batch.decode_sharded(files, F32OracleDecoder()), files)


@pytest.mark.parametrize("chunks", [1, 3])
def test_two_ranks_gloo_f32(chunks):
    """two gloo ranks with a float32 decoder: the buffers, the receive ring and the host copies take the decoder's dtype; the root
    returns float32 PCM equal (in bits) to the one-process result"""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_f32, args=(r, 2, port, q, chunks)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert q.get(timeout=5) == "ok"
