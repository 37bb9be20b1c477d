"""The kernels' arena contract (include/acm_hip.h) at offsets past 32 bits.

include/acm_hip.h gives idx_off, hdr_off, pcm_off and n_emit of a stream descriptor and chunk_off of a second staged form 64 bits, and
the byte-plane arena may be tens of GiB.  tests/test_gpu_arena_contract.py holds every kernel family to the contract on arenas of a few
megabytes that begin at 0; this module runs the same matrix - its CASES, its levels, its check_stats - over far_contract(level)
(tests/arena_contract.py): the same sources, descriptors and residues laid out sparsely, so that

  * staged rows lie astride 2^31 and 2^32 index words (byte 2^32 of the int16 arena is word 2^31) and begin behind them;
  * header runs lie astride header 2^29 (byte 2^32);
  * PCM slots lie astride 2^30, 2^31 and 2^32 elements and begin within 64 elements behind them - as int16 (byte 2^32 is element 2^31)
    and as float32 (element 2^30), which is why float32 stays beside S16LE and U16BE (format conversion is orthogonal to addressing,
    the element size is not);
  * the byte-plane blob and pair table, and the packed blob and chunk table, lie astride byte 2^32 (FarForm).

What an offset comes to with its high bits dropped holds fill or another source's data (the builder asserts it), so a kernel that narrows
an offset on a read computes wrong samples and one that narrows it on a write dirties poison.  Per launch the PCM arena - 16 GiB, one
allocation for all formats - is poisoned, every slot is downloaded and compared with the oracle's slice bit for bit, and EVERY other
word of the arena is checked for poison on the device.  Nothing decodes more than the near test does.

Device memory: 8 GiB of index arena, 4 GiB of headers, 16 to 17.3 GiB of PCM, 4 + 4 GiB of a second form: 38 GiB, held for the module.
The CPU half - the builder's properties, that pieces, descriptors and expectations belong together - is tests/test_arena_contract.py."""
import numpy as np
import pytest

import arena_contract as AC
import helpers  # noqa: F401  (the oracle behind arena_contract's expectations)
from libacm_amd import capi
from test_gpu_arena_contract import CASES, MATRIX, check_stats

pytestmark = pytest.mark.gpu

FORMATS = (capi.FMT_S16LE, capi.FMT_U16BE, AC.F32)
GIB = 1 << 30
NEED = 40 * GIB                 # the most the module holds at once, torch's temporaries of a poison check included
PIECE = GIB                     # bytes of the PCM arena one device-side comparison looks at


class Arenas:
    """the module's device memory: one allocation per arena, grown when a level needs more"""

    def __init__(self, dev):
        self.dev, self.mem, self.pcm = dev, {}, None

    def get(self, name, nbytes):
        ptr, have = self.mem.get(name, (None, 0))
        if have < nbytes:
            self.dev.free(ptr)
            self.mem[name] = (None, 0)
            self.mem[name] = (self.dev.malloc(nbytes), nbytes)
        return self.mem[name][0]

    def pcm_arena(self, nbytes):
        """the PCM arena as a torch tensor of bytes: plans write through its data_ptr(), the poison check reads it in place"""
        import torch
        if self.pcm is None or self.pcm.numel() < nbytes:
            self.pcm = None
            torch.cuda.empty_cache()
            self.pcm = torch.empty((nbytes + (GIB >> 2) - 1) // (GIB >> 2) * (GIB >> 2), dtype=torch.uint8, device="cuda:0")
        return self.pcm

    def close(self):
        import torch
        for ptr, _ in self.mem.values():
            self.dev.free(ptr)
        self.mem, self.pcm = {}, None
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def arenas(dev):
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    if free < NEED:
        pytest.skip("the far arenas need %d bytes of device memory, %d are free" % (NEED, free))
    a = Arenas(dev)
    yield a
    a.close()


def fill_and_upload(dev, ptr, nbytes, fill, pieces, unit):
    """the arena at ptr: `fill` bytes, then the pieces ((offset in units of `unit` bytes, array))"""
    dev.memset(ptr, fill, nbytes)
    for off, a in pieces:
        a = np.ascontiguousarray(a)
        assert off * unit + a.nbytes <= nbytes
        dev.upload(ptr + off * unit, a)


def check_launch(fc, pcm, fmt, what):
    """pcm: the arena (torch bytes) after a launch in format fmt into poison.  Every slot is the oracle's slice, and every other word of
    the arena still holds the poison: compared on the device, in pieces of PIECE bytes"""
    import torch
    f32 = fmt == AC.F32
    view = pcm[:fc.pcm_words * (4 if f32 else 2)].view(torch.int32 if f32 else torch.int16)
    poison = -1 if f32 else AC.POISON16 - 0x10000
    step = PIECE // (4 if f32 else 2)
    pieces = [(a, min(hi, a + step)) for lo, hi in fc.gaps() for a in range(lo, hi, step)]
    dirty = torch.zeros((), dtype=torch.int64, device=pcm.device)
    for a, b in pieces:
        dirty += torch.count_nonzero(view[a:b] != poison)
    ndirty = int(dirty.item())
    if ndirty:
        for a, b in pieces:
            at = torch.nonzero(view[a:b] != poison)
            if at.numel():
                w = a + int(at[0, 0].item())
                raise AssertionError("%s format %s: %d guard words written; the first (0x%x): %s"
                                     % (what, fmt, ndirty, int(view[w].item()) & (0xFFFFFFFF if f32 else 0xFFFF), fc.describe_word(w)))
    for j, (lo, hi, _, _) in enumerate(fc.slots):
        got = view[lo:hi].cpu().numpy().view(np.uint32 if f32 else np.uint16)
        want = fc.expected(j, fmt)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            raise AssertionError("%s format %s: %d samples of a slot differ from the oracle's; the first is sample %d of %s: 0x%x, expected 0x%x"
                                 % (what, fmt, bad.size, bad[0], fc.describe(j), int(got[bad[0]]), int(want[bad[0]])))


@pytest.mark.parametrize("level,name", MATRIX, ids=["%d-%s" % m for m in MATRIX])
def test_plan_keeps_the_contract_far(dev, arenas, level, name):
    import torch
    flags, form, _ = CASES[name]
    fc = AC.far_contract(level)
    ff = AC.far_form(level, form) if form else None
    pcm = arenas.pcm_arena(fc.pcm_words * 4)
    d_idx, d_hdr = arenas.get("idx", fc.idx_words * 2), arenas.get("hdr", fc.hdr_entries * 8)
    fill_and_upload(dev, d_idx, fc.idx_words * 2, AC.FILL, fc.idx_pieces, 2)
    fill_and_upload(dev, d_hdr, fc.hdr_entries * 8, AC.FILL, fc.hdr_pieces, 8)
    if ff:
        d_blob, d_table = arenas.get("blob", ff.blob_bytes), arenas.get("table", ff.table_bytes)
        fill_and_upload(dev, d_blob, ff.blob_bytes, AC.BLOB_FILL, ff.blob_pieces, 1)
        fill_and_upload(dev, d_table, ff.table_bytes, AC.PAIR_FILL if form == "byteplane" else AC.CHUNK_FILL, ff.table_pieces, ff.unit)
    plan = capi.Plan(dev, fc.descs, fc.patches, flags, packed=ff.streams if ff else None)
    try:
        if form == "byteplane":
            plan.bind_mform(d_blob, d_table)
            if name == "byteplane_unbound":
                plan.bind_mform(None, None)
        elif form == "packed":
            plan.bind_packed(d_table, d_blob)
        check_stats(fc, name, plan, plan.stats())
        for fmt in FORMATS[:2] if form == "packed" else FORMATS:
            torch.cuda.synchronize()
            dev.memset(pcm.data_ptr(), 0xFF if fmt == AC.F32 else 0xA5, fc.pcm_words * (4 if fmt == AC.F32 else 2))
            if fmt == AC.F32:
                plan.launch_f32(d_idx, d_hdr, pcm.data_ptr())
            else:
                plan.launch(d_idx, d_hdr, pcm.data_ptr(), fmt)
            dev.sync()
            check_launch(fc, pcm, fmt, "level %d, %s, far:" % (level, name))
    finally:
        plan.destroy()
