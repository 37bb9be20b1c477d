"""The damaged streams of tests/damaged_streams.py through the batch calls on the GPU: acm_batch_decode (both parsers, block ranges,
both staged forms, int16 and float32), its index by-product, acm_batch_index_files and acm_batch_decode_windows.

The batch rule is not the looping decode's: an item ends at its FIRST error (include/acm_hip.h, acm_stage_file) - status = that error,
PCM = the blocks in front of it.  Both are taken from the oracle's plain block-sized reads and checked against what the compiled
reference recorded (tests/golden/ref_answers.json: blocks before the first failing acm_read, its status, the digest of those blocks).
The whole population is one batch with clean base streams between the damaged ones, device-resident in a poisoned arena: a clean
neighbour must come out bit-exact and no word outside the items' own ranges may change.  Nothing here is provoked: a damaged file is
an ordinary input the library must refuse or clip."""
import numpy as np
import pytest

import damaged_streams as D
import helpers  # noqa: F401  (GPU tests run with the fill mode on: helpers sets the switch)
import oracle_api as O
from decode_index import decode_both, index_info
from libacm_amd import capi
from stream_edit import host_index
from test_gpu_batch_index import run as run_batch_index

pytestmark = pytest.mark.gpu

POISON16, POISON32 = 0xA5A5, 0xFFFFFFFF


class Item:
    """one file of the batch and what the batch calls owe for it: status (the open error, the first error, or 0) and pcm (s16le words)"""

    def __init__(self, name, data, status, pcm, opens, clean):
        self.name, self.data, self.status, self.pcm, self.opens, self.clean = name, data, status, pcm, opens, clean


@pytest.fixture(scope="module")
def batch():
    pop, ans, bases = D.population(), D.answers(), D.bases()
    items = []
    for k, (c, a) in enumerate(zip(pop, ans)):
        if a[0] < 0:
            items.append(Item(c.name, c.data, a[0], np.zeros(0, np.uint16), False, False))
        else:
            blocks, status, pcm = D.plain_reads(O.Oracle, c.data, 2 * (c.base.rows << c.base.level))
            assert [blocks, status, D.sha(pcm)] == a[1], c.name             # the oracle's prefix is the reference's
            items.append(Item(c.name, c.data, status, np.frombuffer(pcm, dtype=np.uint16), True, c.kind == "clean"))
        if k % 5 == 4:                  # a clean neighbour
            b = bases[(k // 5) % len(bases)]
            items.append(Item(b.name + ":neighbour", b.data, 0, O.Oracle.decode_all(b.data)[0].view(np.uint16), True, True))
    return items


def device_takes(f):
    """may the device walk of a decode keep this stream?  Clean to its last block, supported, no H1 patch"""
    return host_index(f)[5] and index_info(f).npatches == 0


@pytest.mark.parametrize("f32", [False, True], ids=["s16le", "float32"])
@pytest.mark.parametrize("stage", ["byteplane", "int16"])
@pytest.mark.parametrize("parse,ranges", [(capi.PARSE_HOST, 0), (capi.PARSE_DEVICE, 1), (capi.PARSE_DEVICE, 3)], ids=["host", "device", "device3"])
def test_whole_batch(dev, batch, parse, ranges, stage, f32):
    files = [it.data for it in batch]
    cap = capi.batch_pcm_words(files)
    size = 4 if f32 else 2
    d_pcm = dev.malloc(cap * size)
    try:
        dev.memset(d_pcm, 0xFF if f32 else 0xA5, cap * size)
        flags = (capi.BATCH_STAGE_BYTEPLANE if stage == "byteplane" else capi.BATCH_STAGE_INT16) | (capi.batch_ranges(ranges) if ranges else 0)
        st, words, offs, tm = capi.batch_decode_device(dev, files, d_pcm, cap, threads=4, parse=parse, f32=f32, batch_flags=flags)
        got = np.zeros(cap, np.uint32 if f32 else np.uint16)
        dev.download(got, d_pcm)
    finally:
        dev.free(d_pcm)
    written = np.zeros(cap, bool)
    for k, it in enumerate(batch):
        assert st[k] == it.status, (it.name, st[k], it.status)
        assert words[k] == it.pcm.size, (it.name, words[k], it.pcm.size)
        a, b = offs[k], offs[k] + words[k]
        assert b <= cap and not written[a:b].any(), it.name
        written[a:b] = True
        want = it.pcm.view(np.int16)
        if f32:
            assert np.array_equal(got[a:b].view(np.float32), want.astype(np.float32) * np.float32(2.0 ** -15)), it.name
        else:
            assert np.array_equal(got[a:b].view(np.int16), want), it.name
    assert not (~written & (got != (POISON32 if f32 else POISON16))).any(), "words written outside the items"
    opened = sum(it.opens for it in batch)
    print("n %d  opened %d  first error %d  clean copies %d  device_parsed %d  host_parsed %d  samples %d" % (
        len(batch), opened, sum(it.status != 0 for it in batch if it.opens), sum(it.clean for it in batch), tm.device_parsed, tm.host_parsed, tm.samples))
    assert tm.samples == sum(it.pcm.size for it in batch)
    if parse == capi.PARSE_DEVICE:
        takes = sum(device_takes(it.data) for it in batch if it.opens)
        assert tm.device_parsed + tm.host_parsed == opened
        # an item that fails anywhere, has an H1 patch or ends early is one the host reader parsed again
        assert tm.host_parsed >= opened - takes >= sum(it.status != 0 for it in batch if it.opens)
        assert tm.device_parsed >= 0.9 * sum(it.clean for it in batch)
    else:
        assert (tm.device_parsed, tm.host_parsed) == (0, opened)


@pytest.mark.parametrize("parse", [capi.PARSE_HOST, capi.PARSE_DEVICE], ids=["host", "device"])
def test_index_by_product(dev, batch, parse):
    """acm_batch_decode_indexed on the same batch: every item's marks, blocks and end status are acm_index_file's, byte for byte, and the
    PCM, words and statuses are those of the plain call"""
    got, plain = decode_both(dev, [it.data for it in batch], parse=parse)
    for k, it in enumerate(batch):
        assert got.statuses[k] == it.status and got.words[k] == it.pcm.size, it.name
        assert np.array_equal(got.pcm[k][:it.pcm.size], it.pcm), it.name


def test_batch_index_files(dev, batch):
    """acm_batch_index_files == the host index (marks, blocks, end status, return code), and the device indexes exactly the streams it must"""
    run_batch_index(dev, [it.data for it in batch])


@pytest.mark.parametrize("parse", [capi.PARSE_HOST, capi.PARSE_DEVICE], ids=["host", "device"])
def test_windows_around_the_damage(dev, batch, parse):
    """crops through the host index of damaged items: one that ends in front of the first failing block is ACM_OK and the clean bytes, one
    that reaches it is the clipped slice with the item's end status, one behind it has no words"""
    per_base = {}
    for it in batch:
        if it.opens and it.status != 0 and it.pcm.size >= 64:
            per_base.setdefault(it.name.split(":")[0], []).append(it)
    chosen = [it for name in sorted(per_base) for it in per_base[name][::max(1, len(per_base[name]) // 3)][:3]]
    assert len(chosen) >= 35 and len(per_base) >= 14
    files = [it.data for it in chosen]
    index = [capi.index_file(f)[0] for f in files]
    windows, want = [], []
    for k, it in enumerate(chosen):
        w, bl = it.pcm.size, index_info(it.data).rows * index_info(it.data).cols
        assert index[k].end_status == it.status
        first = max(0, w - bl - 30)
        for first, count, status in ((first, w - 30 - first, 0), (w - 50, 200, it.status), (w + 5, 100, it.status), (0, w + 1, it.status)):
            windows.append((k, first, count))
            want.append((status, it.pcm[first:first + count]))
    res, tm = capi.batch_decode_windows(dev, files, index, windows, parse=parse, threads=4)
    for (k, first, count), (status, pcm), (got_status, got_words, got) in zip(windows, want, res):
        assert (got_status, got_words) == (status, pcm.size), (chosen[k].name, first, count, got_status, got_words)
        assert np.array_equal(got, pcm), (chosen[k].name, first, count)
