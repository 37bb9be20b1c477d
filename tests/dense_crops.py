"""The cases of the dense crop batches (acm_batch_decode_windows_dense, include/acm_hip.h), for tests/test_dense_crops.py (the row table
and the cases' own coverage, without a GPU) and tests/test_gpu_dense_crops.py (the call itself).

A handful of small synthetic files - level 1 (two columns), 5 and 9, mono and stereo, streams that end inside a block, one cut off in
the middle of its bytes, one blob that is not ACM - and, per channel count and row length, one list of windows over them.  What a row
must hold is computed here from the oracle's whole-file decode by the formula of the contract, in numpy; what a window must report
comes from tests/test_block_index.py::expected_window, the rule the windows call is held to."""
from types import SimpleNamespace

import numpy as np

from helpers import make_stream, oracle_pcm
from libacm_amd import capi
from test_block_index import expected_window

ACM_ERR_NOT_ACM = -3
FRAMES = (64, 37)               # a row length that is a multiple of 8 for either channel count, and one that is not


class File:
    """a file image, its index and what the host parser and the oracle say about it"""

    def __init__(self, data):
        self.data = data
        self.rc, self.info = capi.probe(data)
        self.acm = self.rc == 0
        self.st = capi.stage_file(data) if self.acm else None
        self.marks, self.ix = capi.index_file(data) if self.acm else (None, None)
        self.channels = self.info.channels if self.acm else 0
        self.pcm = oracle_pcm(data)[0].view(np.int16) if self.acm else np.zeros(0, np.int16)
        self.words = self.st.words if self.acm else 0
        assert self.pcm.size == self.words
        self.end_status = self.st.info.end_status if self.acm else self.rc


_files = None


def files():
    global _files
    if _files is None:
        whole = make_stream(9105, 5, 4, 12)
        _files = [File(d) for d in (
            make_stream(9100, 1, 16, 20),                       # 0: level 1 - two columns: a window's lead is 0 or 1 - mono, 640 samples
            make_stream(9101, 1, 8, 30, channels=2),            # 1: level 1, stereo
            make_stream(9102, 5, 4, 12, cut=37),                # 2: level 5, mono, total_values ends inside the last block
            make_stream(9103, 5, 3, 16, channels=2, cut=41),    # 3: level 5, stereo, blocks of an odd height, an odd total_values
            make_stream(9104, 9, 2, 4),                         # 4: level 9, mono
            make_stream(9106, 9, 2, 4, channels=2, cut=301),    # 5: level 9, stereo, cut inside a block
            whole[:len(whole) * 2 // 3],                        # 6: cut off in the middle of its bytes: an error end status
            b"not an acm file, whatever its length is",         # 7
        )]
        assert [f.channels for f in _files] == [1, 2, 1, 2, 1, 2, 1, 0]
        assert _files[6].end_status < 0 < _files[6].words and _files[2].words % _files[2].st.block_len and not _files[7].acm
        assert all(f.words % 2 == 0 for f in _files if f.channels == 2)
    return _files


class Case:
    """one call: `windows` over files() as rows of frames * channels samples"""

    def __init__(self, channels, frames, windows):
        self.channels, self.frames, self.windows = channels, frames, windows
        self.row = channels * frames
        self.name = "c%d_t%d" % (channels, frames)

    def rejected(self, k):
        """turned away softly for its channel count"""
        f = self.windows[k][0]
        return f < len(files()) and files()[f].acm and files()[f].channels != self.channels

    def delivers(self, k):
        """samples of `whole` window k holds: none for a window turned away, of a file that is not ACM or of no file at all"""
        f, first, count = self.windows[k]
        if f >= len(files()) or self.rejected(k):
            return 0
        return max(0, min(count, files()[f].words - first))

    def expect(self, k):
        """(words, status, blocks staged) the call reports for window k"""
        f, first, count = self.windows[k]
        if f >= len(files()) or self.rejected(k):
            return 0, capi.ERR_ARG, 0
        words, status, b0, nb = expected_window(files()[f].st, files()[f].rc, first, count)
        return words, status, nb

    def rows(self, planar):
        """the expected tensor, int16 [N, row]: the contract's formula"""
        out = np.zeros((len(self.windows), self.row), np.int16)
        for k, (f, first, count) in enumerate(self.windows):
            words = self.delivers(k)
            out[k, :words] = files()[f].pcm[first:first + words] if words else 0
        if planar:
            out = out.reshape(-1, self.frames, self.channels).transpose(0, 2, 1).reshape(-1, self.row)
        return np.ascontiguousarray(out)


def as_f32(i16):
    return i16.astype(np.float32) * np.float32(2.0 ** -15)


def build_case(channels, frames):
    C, R = channels, channels * frames
    rng = np.random.default_rng([0xDE5E, channels, frames])
    wins = []
    for f, src in enumerate(files()):
        if src.channels != C or f == 6:
            continue
        W, bl = src.words, src.st.block_len
        assert W > 8 * 11 + R + 8
        wins += [(f, 8 * (3 + r) + r, R) for r in range(0, 8, C)]               # every residue of first_word % 8 a multiple of C can have
        wins += [(f, 5 * C, 0), (f, 6 * C, C), (f, 4 * C, 8), (f, 17 * C, R - C), (f, 9 * C, R)]
        if C == 1:
            wins += [(f, 11, 7), (f, 13, 9)]
        wins += [(f, W + 3 * C, 4 * C),                                         # starts behind the end
                 (f, W - 5 * C, R),                                             # clipped by the end
                 (f, bl - 3 * C, 8 * C)]                                        # across a block boundary
        for _ in range(6):
            n = C * int(rng.integers(1, frames + 1))
            wins.append((f, C * int(rng.integers(0, (W - n) // C + 1)), n))
    if C == 1:
        W = files()[6].words                                                    # the file that breaks off: whole windows, and its own status at the end
        wins += [(6, 3, R), (6, W - 8, R), (6, W + 1, 4)]
    other = 0 if C == 2 else 3
    wins += [(7, 0, R), (7, 4 * C, 0),                                          # not ACM
             (99, 0, 4 * C),                                                    # no such file
             (other, 8 * C, R), (other, 2, 0)]                                  # the other channel count
    return Case(C, frames, wins)


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = [build_case(c, t) for c in (1, 2) for t in FRAMES]
    return _cases


def index_of(fs=None):
    return [f.marks for f in (fs or files())]


def layout_item(f):
    """a file as tests/test_window_layout.py describes one to the layout hooks and to its model"""
    if not f.acm:
        info = SimpleNamespace(level=0, rows=0, cols=0, channels=0, total_values=0, header_bytes=0, blocks=0, end_status=0)
        return SimpleNamespace(info=info, len=len(f.data), ok=0, end_status=f.rc, whole=0, marks=None, st=None)
    i = f.info
    info = SimpleNamespace(level=i.level, rows=i.rows, cols=i.cols, channels=i.channels, total_values=i.total_values, header_bytes=i.header_bytes,
                           blocks=f.ix.blocks, end_status=f.ix.end_status)
    return SimpleNamespace(info=info, len=len(f.data), ok=1, end_status=f.ix.end_status, whole=f.words, marks=np.asarray(f.marks), st=f.st)
