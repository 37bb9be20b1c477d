"""Batch-of-files front end across the GPUs of one node (BASELINE.json north_star).

One process per GPU (torch.distributed; backend "nccl" = RCCL over xGMI on ROCm, "gloo" in CPU tests).
ACM streams share no state, so the data path has NO collective:

    rank 0:  read the 14-byte headers -> weights (total_values) -> greedy longest-first shards
    C1    :  scatter of the shard TABLE - file ids and paths, a few KB; never file contents   [collective, control]
    C1b   :  every rank's chunk plan (PCM capacity per chunk, from headers and file lengths) to rank 0   [control]
    rank r:  read its own files, parse and synthesise them on its GPU chunk by chunk; chunk k travels to rank 0
             point-to-point (2 B/sample, straight from the buffer the decoder filled) while chunk k + 1 decodes
    rank 0:  decodes its own chunks and receives the others' into a ring of device buffers -> pinned host memory
    C3    :  per-stream status, offsets and word counts to rank 0 (gather_object) once the transfers are done  [results]

The decode itself is injected (`decoder`): the product decoder is GpuDecoder below (HIP kernels through
libacm_hip.so, device memory owned by torch); tests on CPU-only machines inject a stand-in so that
sharding, scatter and gather are exercised with world_size > 1.
"""
import heapq
import math
import os

import numpy as np

from . import capi


def shard_longest_first(weights, n_ranks):
    """Greedy LPT: heaviest stream first onto the least loaded rank.  Returns n_ranks lists of indices."""
    shards = [[] for _ in range(n_ranks)]
    heap = [(0, r) for r in range(n_ranks)]
    heapq.heapify(heap)
    for i in sorted(range(len(weights)), key=lambda k: (-weights[k], k)):
        load, r = heapq.heappop(heap)
        shards[r].append(i)
        heapq.heappush(heap, (load + weights[i], r))
    return shards


def file_weight(data):
    """Decode cost proxy known from the 14-byte header alone: total_values (0 for non-ACM files)."""
    rc, info = capi.probe(data)
    return int(info.total_values) if rc == 0 else 0


def _is_path(f):
    return isinstance(f, (str, os.PathLike))


def _head(f, n=64):
    """the first bytes of a file (path) or file image (bytes): enough for the ACM / WAVC header"""
    if _is_path(f):
        with open(f, "rb") as fh:
            return fh.read(n)
    return bytes(f[:n])


def _load(f):
    if _is_path(f):
        with open(f, "rb") as fh:
            return fh.read()
    return f


def pcm_capacity_words(head, file_len, force_chans=0):
    """16-bit words a stream can take in the dense PCM buffer of a decode call, from its header and its length alone - what
    acm_batch_pcm_words() adds up (acm_batch.cpp: blocks_possible): the blocks the header promises, but no more than the bytes
    of the file can hold (a block costs at least its 20-bit header and a 5-bit filler code per column, decode.c:491-502,
    586-589), padded to 64 words.  0 for a file that is not ACM."""
    rc, info = capi.probe(head, force_chans)
    if rc != 0:
        return 0
    bl = info.rows * info.cols
    promised = (info.total_values + bl - 1) // bl
    bits = max(0, file_len - info.header_bytes) * 8 + 8
    blocks = min(promised, bits // (20 + 5 * info.cols) + 1)
    return (blocks * bl + 63) // 64 * 64


def build_index(files, threads=0, decoder=None):
    """The block index of every file (capi.index_file: start bit, val and pwr of each block - 16 bytes per block), built once on the
    host and kept: GpuDecoder.crop() takes it back on every call.  (Files that are decoded whole anyway need no pass of their own:
    GpuDecoder.__call__(files, return_index=True) hands the same index out beside the PCM.)  files: paths or file images.  Returns a list of numpy record arrays
    (capi.BlockIndex: capi.BLOCK_MARK_DT records that also remember how the stream ends; np.save / np.load keep the records), an empty
    one for a file that is not ACM.  threads: 0 = one per CPU, at most 64.
    decoder: a GpuDecoder - the index is built through its device handle (GpuDecoder.build_index: the device walks the clean streams
    where that pays, the same marks either way); None: the host parser, file by file."""
    from concurrent.futures import ThreadPoolExecutor
    if decoder is not None:
        return decoder.build_index(files, threads=threads)

    def one(f):
        try:
            return capi.index_file(_load(f))[0]
        except ValueError:
            return np.zeros(0, dtype=capi.BLOCK_MARK_DT)
    workers = threads if threads > 0 else min(64, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
    with ThreadPoolExecutor(max_workers=max(1, workers)) as ex:         # (the parsing runs inside the library: the GIL is released)
        return list(ex.map(one, files))


class GpuDecoder:
    """Decode a list of file images on this rank's GPU; PCM stays in HBM as one torch int16 tensor.

    dtype=torch.float32: the tensor holds float32 samples instead, each the s16le sample times 2^-15 exactly (in [-1, 1), what
    torchaudio.load returns), written by the synthesis kernels themselves (ACM_BATCH_PCM_F32: fmt must stay FMT_S16LE).
    Device memory and the stream belong to torch (plumbing); parsing and synthesis are libacm_hip.so's.
    """

    def __init__(self, ordinal=None, fmt=capi.FMT_S16LE, parse=capi.PARSE_AUTO, dtype=None):
        import torch
        self.torch = torch
        if ordinal is None:
            ordinal = torch.cuda.current_device()
        self.dtype = torch.int16 if dtype is None else dtype
        if self.dtype not in (torch.int16, torch.float32):
            raise ValueError("GpuDecoder: dtype torch.int16 or torch.float32, not %s" % (self.dtype,))
        if self.dtype == torch.float32 and fmt != capi.FMT_S16LE:
            raise ValueError("GpuDecoder: float32 samples are the s16le ones scaled; fmt must be FMT_S16LE")
        self.ordinal = ordinal
        self.fmt = fmt
        self.parse = parse
        self.timing = None
        self.index_timing = None
        self._chans = None              # crop_batch(mix=True): (the index object, channels per file of the files it belongs to)
        self._rates = None              # crop_batch(rate=...): (the index object, sample rate per file)
        torch.cuda.set_device(ordinal)
        # the library runs on a stream of its own (torch's current stream is usually the null stream, which
        # acmhip_device_open does not adopt); __call__ orders the two around the torch-owned PCM tensor
        self.dev = capi.Device(ordinal)

    def empty(self, words):
        """a PCM buffer this decoder can decode into (decode_sharded keeps two of them per rank and reuses them)"""
        return self.torch.empty(max(words, 1), dtype=self.dtype, device="cuda:%d" % self.ordinal)

    def __call__(self, files, out=None, return_index=False):
        """-> (pcm tensor in HBM - int16, or float32 -, per-file sample offsets into it, per-file sample counts, per-file statuses).
        out: a tensor of this decoder's dtype of at least acm_batch_pcm_words(files) samples to decode into (else a new one is allocated).
        return_index=True: a fifth element, the block index of every file as build_index(files) returns it - a by-product of this
        decode's own parse (acm_batch_decode_indexed: no stream is walked a second time), ready for crop()"""
        torch = self.torch
        cap = capi.batch_pcm_words(files)
        if out is not None and out.dtype != self.dtype:
            raise ValueError("GpuDecoder: out is %s, the decoder writes %s" % (out.dtype, self.dtype))
        d_pcm = out if out is not None and out.numel() >= cap else torch.empty(max(cap, 1), dtype=self.dtype, device="cuda")
        # a block the caching allocator hands out may still be in use by torch work queued on torch's stream
        torch.cuda.current_stream().synchronize()
        # one call: threaded (or device-side) bit parsing, pipelined H2D, synthesis; the PCM stays in d_pcm.  In steady state
        # nothing in it allocates or frees device memory (grow-only arenas, plan tables from the handle's spare blocks), so a
        # transfer of the previous chunk that is still in flight is not waited for
        res = capi.batch_decode_device(
            self.dev, files, d_pcm.data_ptr(), d_pcm.numel(), fmt=self.fmt, parse=self.parse, f32=self.dtype == torch.float32, index=return_index)
        statuses, words, offsets, self.timing = res[:4]
        # acm_batch_decode returns with its stream drained: d_pcm is complete and visible to torch's streams
        return (d_pcm, offsets, words, statuses) + tuple(res[4:])


    def build_index(self, files, threads=0, parse=None, max_group_bytes=0):
        """The block index of every file, as batch.build_index(files) returns it, through acm_batch_index_files: the device walks the
        clean streams and writes 16 bytes per block (parse=capi.PARSE_DEVICE; the decoder's own parse mode by default), the host pool
        indexes what the device is not sure about.  self.index_timing: the call's capi.IndexTiming."""
        files = [_load(f) for f in files]
        index, self.index_timing = capi.batch_index_files(self.dev, files, parse=self.parse if parse is None else parse,
                                                          max_group_bytes=max_group_bytes, threads=threads)
        return index

    def crop(self, files, windows, index=None, out=None):
        """Random-access crops: windows = (file_no, first_sample, n_samples) triples over interleaved samples, index = build_index(files)
        (None: built here, through this decoder - keep it where more than one call crops the same files).
        Only the blocks a window needs are parsed, uploaded and synthesised.
        -> (pcm tensor in HBM of this decoder's dtype, per-window offsets of the first requested sample, per-window sample counts,
        per-window statuses).  Window k is pcm[offsets[k] : offsets[k] + counts[k]] = the whole decode's [first : first + n], clipped to
        the end of the stream."""
        torch = self.torch
        files = [_load(f) for f in files]
        if index is None:
            index = self.build_index(files)
        cap = capi.batch_window_pcm_words(files, windows)
        if out is not None and out.dtype != self.dtype:
            raise ValueError("GpuDecoder: out is %s, the decoder writes %s" % (out.dtype, self.dtype))
        d_pcm = out if out is not None and out.numel() >= cap else torch.empty(max(cap, 1), dtype=self.dtype, device="cuda:%d" % self.ordinal)
        torch.cuda.current_stream().synchronize()
        statuses, words, offsets, _, self.timing = capi.batch_decode_windows_device(
            self.dev, files, index, windows, d_pcm.data_ptr(), d_pcm.numel(), fmt=self.fmt, parse=self.parse, f32=self.dtype == torch.float32)
        return d_pcm, offsets, words, statuses

    def _header_channels(self, files, index):
        """[f]: 1 or 2, the channel count the header of files[f] says, 0 for a file without one.  Read once per index: the counts are
        as permanent as the block index that belongs to the same files, so they are kept with the index object of the last call and a
        step that crops the same files with the same index reads no header again"""
        kept = self._chans
        if kept is None or kept[0] is not index or len(kept[1]) != len(files):
            found = capi.header_channels(files)
            kept = self._chans = (index, [found[f] if found.get(f) in (1, 2) else 0 for f in range(len(files))])
        return kept[1]

    def _header_rates(self, files, index):
        """[f]: the sample rate the header of files[f] says, None for a file without one; kept with the index object as the channel
        counts are"""
        kept = self._rates
        if kept is None or kept[0] is not index or len(kept[1]) != len(files):
            found = capi.header_rates(files)
            kept = self._rates = (index, [found.get(f) for f in range(len(files))])
        return kept[1]

    def _sources(self, name, files, windows, channels, index, mix, rate, speed, responses=None, reverb=None):
        """what the three crop_* methods (`name` is the one that asks) do with their source windows before the call: the checks of
        speed and reverb, the files loaded, the index, the samples per frame of every window's file - its own header's with mix (a
        file without one is checked as the batch's kind) -, the header rates where the call resamples, the windows in samples and the
        filter's keywords.  -> (files, index, per, rates, scaled windows, fir keywords)"""
        if reverb is not None and responses is None:
            raise ValueError("GpuDecoder.%s: reverb needs responses" % name)
        if reverb is not None and len(reverb) != len(windows):
            raise ValueError("GpuDecoder.%s: reverb has %d entries for %d windows" % (name, len(reverb), len(windows)))
        files = [_load(f) for f in files]
        if index is None:
            index = self.build_index(files)
        per = [channels] * len(windows)
        if mix:
            own = self._header_channels(files, index)
            per = [own[w[0]] or channels if w[0] < len(files) else channels for w in windows]
        if speed is not None and rate is None:
            raise ValueError("GpuDecoder.%s: speed needs rate" % name)
        rates = self._header_rates(files, index) if rate is not None else None
        fir = {}
        if responses is not None:
            fir = dict(responses=[r.record for r in responses], of_window=reverb if reverb is not None else [None] * len(windows))
        return files, index, per, rates, [(f, first * c, count * c) for (f, first, count), c in zip(windows, per)], fir

    def _output(self, out, need, dtype, mismatch):
        """the flat tensor a call writes `need` elements of `dtype` into: `out` where it is contiguous and large enough, else a new
        one; torch's stream is drained, since a block the caching allocator hands out may still be in use by work queued on it"""
        if out is not None and out.dtype != dtype:
            raise ValueError(mismatch % (out.dtype,))
        fits = out is not None and out.numel() >= need and out.is_contiguous()
        d_out = out if fits else self.torch.empty(max(need, 1), dtype=dtype, device="cuda:%d" % self.ordinal)
        self.torch.cuda.current_stream().synchronize()
        return d_out

    @staticmethod
    def _row_table(rows):
        """the overlay row table in one piece: an Overlay has made its record when it was built"""
        table = np.zeros(len(rows), dtype=capi.OVERLAY_ROW_DT)
        if len(rows):
            table.view(np.uint32).reshape(len(rows), -1)[:, :5] = np.array([r.raw for r in rows], dtype=np.uint32)
        return table

    @staticmethod
    def _delivered(words, per, windows, rates, rate, speed):
        """frames every row got, from the samples its window delivered: the window's own frames, or the output frames of a row that
        is resampled (a row that got frames is of a file with a rate the filter takes)"""
        delivered = [w // c for w, c in zip(words, per)]
        if speed is not None:
            # (a batch has a handful of distinct (frames, rate, speed): each is asked of the library once)
            known = {}
            for k, (d, w, sp) in enumerate(zip(delivered, windows, speed)):
                if d:
                    sp = tuple(sp) if sp else (1, 1)
                    key = (d, rates[w[0]], sp)
                    if key not in known:
                        known[key] = capi.dense_speed_frames(d, rates[w[0]], rate, sp)
                    delivered[k] = known[key]
        elif rate is not None:
            delivered = [capi.dense_resampled_frames(d, rates[w[0]], rate) if d else 0 for d, w in zip(delivered, windows)]
        return delivered

    def crop_batch(self, files, windows, frames, channels=1, planar=True, index=None, out=None, mix=False, rate=None, speed=None):
        """Random-access crops as one batch tensor: windows = (file_no, first_frame, n_frames) triples with n_frames <= frames, index as
        for crop().  -> (batch, frames_delivered, statuses): batch is a tensor of this decoder's dtype shaped [N, channels, frames]
        (planar) or [N, frames, channels], row k the crop's frames with zeros behind them - also where a window is clipped by the end of
        its stream, starts behind it, or is turned away: a file that is not ACM, a stale index, a file whose channel count is not
        `channels` (status capi.ERR_ARG).  One copy kernel behind the synthesis lays the rows out (acm_batch_decode_windows_dense); no
        per-window slicing on the torch side.  out: a contiguous tensor of this decoder's dtype with at least N * channels * frames
        elements is written into (the batch is a view of its first elements) instead of a new one, as in crop().
        mix=True (ACM_DENSE_MIX): mono and stereo files in one batch.  Windows are (file_no, first_frame, n_frames) for any file; a file
        with the other channel count is decoded and converted instead of turned away - stereo becomes (L + R) >> 1, a mono sample goes
        into both channels - and frames_delivered counts its frames.  The channel counts are read from the headers once per `index`
        object and kept with it: pass the index of the files, and a new one with new files, as crop() needs anyway.
        rate (ACM_DENSE_RESAMPLE): the batch's sample rate.  Windows stay (file_no, first_frame, n_frames) in the file's own frames at
        its own rate - source_frames() says how many fit a row; the row of a file at another rate is its crop resampled, zeros beyond
        the crop's ends, and frames_delivered[k] counts the row's OUTPUT frames.  A file whose ratio to `rate` the filter does not take
        is turned away (capi.ERR_ARG).  The rates are kept with the index object, beside the channel counts.
        speed (ACM_DENSE_SPEED, with rate): a (num, den) pair per window, or None for 1/1 - window k is played at num / den (11/10:
        faster, fewer frames), which is a resampling of its own; any ratio down to an eighth is taken, the odd ones by a filter that
        interpolates between prototype phases.  source_frames(..., speed=) says how long a window fits a row."""
        files, index, per, rates, scaled, _ = self._sources("crop_batch", files, windows, channels, index, mix, rate, speed)
        n = len(windows)
        shape = (n, channels, frames) if planar else (n, frames, channels)
        need = n * channels * frames
        d_pcm = self._output(out, need, self.dtype, "GpuDecoder: out is %%s, the decoder writes %s" % (self.dtype,))
        statuses, words, self.timing = capi.batch_decode_windows_dense(
            self.dev, files, index, scaled, d_pcm.data_ptr(), d_pcm.numel(), frames, channels=channels, planar=planar, fmt=self.fmt,
            parse=self.parse, f32=self.dtype == self.torch.float32, mix=mix, rate=rate, speeds=speed)
        # the call returns with its stream drained: the batch is complete and visible to torch's streams
        return d_pcm.reshape(-1)[:need].view(shape), self._delivered(words, per, windows, rates, rate, speed), statuses

    def crop_overlay(self, files, windows, rows, frames, channels=1, planar=True, index=None, out=None, mix=False, rate=None, speed=None,
                     responses=None, reverb=None):
        """crop_batch with volume perturbation and an overlay at a signal-to-noise ratio in the same call
        (acm_batch_decode_windows_overlay).  windows, frames, channels, planar, index, mix, rate and speed are crop_batch's and define
        the SOURCE rows - what crop_batch would return, kept in memory of the decoder's own.  rows: one Overlay per row of the batch:
        source row a, scaled by vol_db, with source row b laid over it at snr_db (a's power over b's, measured over the whole rows) or
        at gain_db.  Sources may be used by many rows, by none, in any order.
        -> (batch [len(rows), channels, frames] (planar) or [len(rows), frames, channels], gains, frames_delivered, statuses): gains[r]
        is (g, energy_a, energy_b), the Q12 gain b got and the sums of squares it was made from; frames_delivered and statuses are
        the WINDOWS', as crop_batch reports them.  The result is defined on integers (include/acm_hip.h), float32 is the int16 result
        times 2^-15; out as in crop_batch.
        responses, reverb (acm_batch_decode_windows_overlay_fir): a list of Response, and per window the number of the one its source
        row is convolved with before anything else is made from it - energies included, so the noise is set against the reverberant
        speech - or None for a window that stays dry.  The row keeps its length: a crop's tail rings on into the zeros behind it."""
        files, index, per, rates, scaled, fir = self._sources("crop_overlay", files, windows, channels, index, mix, rate, speed, responses, reverb)
        nr = len(rows)
        shape = (nr, channels, frames) if planar else (nr, frames, channels)
        need = nr * channels * frames
        d_pcm = self._output(out, need, self.dtype, "GpuDecoder: out is %%s, the decoder writes %s" % (self.dtype,))
        call = capi.batch_decode_windows_overlay_fir if responses is not None else capi.batch_decode_windows_overlay
        statuses, words, _, gains, self.timing = call(
            self.dev, files, index, scaled, self._row_table(rows), d_pcm.data_ptr(), d_pcm.numel(), frames, channels=channels, planar=planar,
            fmt=self.fmt, parse=self.parse, f32=self.dtype == self.torch.float32, mix=mix, rate=rate, speeds=speed, **fir)
        return d_pcm.reshape(-1)[:need].view(shape), gains, self._delivered(words, per, windows, rates, rate, speed), statuses

    def crop_features(self, files, windows, frames, bank, rows=None, index=None, out=None, mix=False, rate=None, speed=None, responses=None,
                      reverb=None, log=None):
        """mel filterbank features of the batch crop_overlay would make, in the same call (acm_batch_decode_windows_features): the
        waveform - mono, int16, `frames` samples a row - stays in memory of the decoder's own and only the features are written.
        windows, frames, index, mix, rate, speed, responses and reverb are crop_overlay's; rows: one Overlay per row, by default
        Overlay(k) for every window k; bank: a MelBank.
        -> (feats, gains, frames_delivered, statuses): feats float32 [len(rows), n_mels, F] - [len(rows), F, n_mels] for a time-major
        bank - with F = bank.frames(frames), whatever the decoder's dtype; the rest as crop_overlay returns it.  The features are
        defined on integers (include/acm_hip.h): (32639 / 32768)^2 times the power mel spectrogram of the row / 32768, frames padded
        with zeros.  out as in crop_overlay, but float32.
        log (acm_batch_decode_windows_logmel): a LogScale - feats is then the logarithm of those features, floored, clamped to the
        row's maximum where the scale has a top, and scaled, still defined on integers and made in the same call:
        log=LogScale.whisper() is log10, clamp(min=1e-10), maximum(amax - 8), (x + 4) / 4.  A scale the library does not take is a
        ValueError."""
        files, index, per, rates, scaled, fir = self._sources("crop_features", files, windows, 1, index, mix, rate, speed, responses, reverb)
        if rows is None:
            rows = [Overlay(k) for k in range(len(windows))]
        nr = len(rows)
        F = bank.frames(frames)
        shape = (nr, F, bank.n_mels) if bank.time_major else (nr, bank.n_mels, F)
        need = nr * bank.n_mels * F
        d_out = self._output(out, need, self.torch.float32, "GpuDecoder.crop_features: out is %s, the features are float32")
        if log is not None:
            if capi.feat_log_check(bank.record, log.record) != 0:
                raise ValueError("GpuDecoder.crop_features: a LogScale acm_feat_log_check does not take: %r" % (log.record,))
            fir = dict(fir, log=capi.feat_log(*log.record))
        statuses, words, _, gains, self.timing = capi.batch_decode_windows_features(
            self.dev, files, index, scaled, self._row_table(rows), d_out.data_ptr(), d_out.numel(), frames, bank.record, channels=1, planar=True,
            fmt=self.fmt, parse=self.parse, f32=False, mix=mix, rate=rate, speeds=speed, **fir)
        return d_out.reshape(-1)[:need].view(shape), gains, self._delivered(words, per, windows, rates, rate, speed), statuses


class MelBank:
    """the tables of GpuDecoder.crop_features (acm_feat_bank): a periodic Hann window of win_length samples (n_fft by default) centred
    in n_fft, the DFT's cosines and n_mels HTK mel triangles from f_min to f_max (rate / 2 by default), quantised by acm_feat_design.
    center: frame f is centred on sample f * hop and a row of T samples has 1 + T // hop frames, zeros outside the row (torch.stft
    with pad_mode="constant"); else only whole frames count.  time_major: features as [row, frame, band]."""

    def __init__(self, rate, n_fft=512, win_length=None, hop=160, n_mels=80, f_min=0.0, f_max=None, center=True, time_major=False):
        flags = (capi.FEAT_CENTER if center else 0) | (capi.FEAT_TIME_MAJOR if time_major else 0)
        tables = capi.feat_design(rate, n_fft, win_length, hop, n_mels, f_min, f_max, flags)
        self._set(n_fft, hop, n_mels, flags, *tables)

    def _set(self, n_fft, hop, n_mels, flags, window, cs, mel_first, mel_count, mel_off, mel_w):
        self.n_fft, self.hop, self.n_mels, self.flags = n_fft, hop, n_mels, flags
        self.center, self.time_major = bool(flags & capi.FEAT_CENTER), bool(flags & capi.FEAT_TIME_MAJOR)
        self.window, self.cs, self.mel_first, self.mel_count, self.mel_off, self.mel_w = window, cs, mel_first, mel_count, mel_off, mel_w
        self.record = (n_fft, hop, n_mels, flags, window, cs, mel_first, mel_count, mel_off, mel_w)    # as capi.feat_bank takes them

    @classmethod
    def raw(cls, n_fft, hop, window, cs, mel_first, mel_count, mel_off, mel_w, center=True, time_major=False):
        """a MelBank of integer tables as they are (include/acm_hip.h has their ranges); n_mels is len(mel_first).  What
        acm_feat_bank_check does not take is a ValueError"""
        def table(a, dt, lo, hi):
            a = np.asarray(a)
            if a.ndim != 1 or (a.size and ((a != np.rint(a)).any() or a.min() < lo or a.max() > hi)):
                raise ValueError("MelBank.raw: a table of integers in [%d, %d]" % (lo, hi))
            return a.astype(dt)
        b = cls.__new__(cls)
        flags = (capi.FEAT_CENTER if center else 0) | (capi.FEAT_TIME_MAJOR if time_major else 0)
        b._set(int(n_fft), int(hop), len(mel_first), flags, table(window, "<i2", -32768, 32767), table(cs, "<i2", -32768, 32767),
               table(mel_first, "<u2", 0, 65535), table(mel_count, "<u2", 0, 65535), table(mel_off, "<u4", 0, 2 ** 32 - 1),
               table(mel_w, "<u2", 0, 65535))
        if b.window.size != b.n_fft or b.cs.size != b.n_fft or not b.mel_count.size == b.mel_off.size == b.n_mels or \
                (b.n_mels and int(np.where(b.mel_count > 0, b.mel_off.astype(np.int64) + b.mel_count, 0).max()) > b.mel_w.size):
            raise ValueError("MelBank.raw: tables of n_fft, n_fft, n_mels, n_mels, n_mels entries, and every band's weights")
        if capi.feat_bank_check(*b.record) != 0:
            raise ValueError("MelBank.raw: a bank acm_feat_bank_check does not take")
        return b

    def frames(self, T):
        """F: the frames of a row of T samples"""
        return capi.feat_frames(T, self.n_fft, self.hop, self.flags)


class LogScale:
    """the logarithm GpuDecoder.crop_features(log=) ends with (acm_feat_log): post_mul * log(max(y, floor)) + post_add of the linear
    feature y, log being ln, log2, log10 or - "db" - 10 log10; with top, nothing more than `top` (in the logarithm's own unit, before
    post_mul) below the largest value of its row.  The library works on log2 y in Q16: mul_q24 = nearbyint(2^24 * c * post_mul) with
    c = 1, ln 2, log10 2 or 10 log10 2, floor_q16 = nearbyint(65536 * log2(floor)), top_q16 = nearbyint(65536 * top / c), offset_q16 =
    nearbyint(65536 * post_add)."""
    KINDS = {"log2": 1.0, "ln": math.log(2.0), "log10": math.log10(2.0), "db": 10.0 * math.log10(2.0)}

    def __init__(self, kind="ln", floor=1e-10, top=None, post_mul=1.0, post_add=0.0):
        if kind not in self.KINDS:
            raise ValueError("LogScale: kind is one of %s" % ", ".join(sorted(self.KINDS)))
        if not floor > 0 or (top is not None and top < 0):
            raise ValueError("LogScale: a floor above 0 and a top of 0 or more")
        c = self.KINDS[kind]
        self._set(capi.FEAT_LOG_TOP if top is not None else 0, int(np.rint(65536 * math.log2(floor))), int(np.rint(2.0 ** 24 * c * post_mul)),
                  int(np.rint(65536 * post_add)), 0 if top is None else int(np.rint(65536 * top / c)))
        self.kind = kind

    def _set(self, flags, floor_q16, mul_q24, offset_q16, top_q16):
        self.kind = None
        self.flags, self.floor_q16, self.mul_q24, self.offset_q16, self.top_q16 = flags, floor_q16, mul_q24, offset_q16, top_q16
        self.record = (flags, floor_q16, mul_q24, offset_q16, top_q16)          # as capi.feat_log takes them
        for v, lo, hi in ((flags, 0, 2 ** 32 - 1), (floor_q16, -2 ** 31, 2 ** 31 - 1), (mul_q24, 0, 2 ** 32 - 1), (offset_q16, -2 ** 31, 2 ** 31 - 1),
                          (top_q16, 0, 2 ** 32 - 1)):
            if not lo <= v <= hi:
                raise ValueError("LogScale: %r is no field of acm_feat_log" % (v,))

    @classmethod
    def whisper(cls):
        """log10, floor 1e-10, the row's maximum less 8, (x + 4) / 4"""
        return cls("log10", 1e-10, 8.0, 0.25, 1.0)

    @classmethod
    def raw(cls, floor_q16, mul_q24=1 << 24, offset_q16=0, top_q16=None):
        """a LogScale of acm_feat_log's integer fields as they are (include/acm_hip.h has their ranges); top_q16 None: no top"""
        g = cls.__new__(cls)
        g._set(capi.FEAT_LOG_TOP if top_q16 is not None else 0, int(floor_q16), int(mul_q24), int(offset_q16), 0 if top_q16 is None else int(top_q16))
        return g


def snr_q16(db):
    """a signal-to-noise ratio in dB as acm_overlay_row.snr: the power ratio in Q16, 1 .. 2^32 - 1"""
    return min(max(int(round(65536 * 10 ** (db / 10))), 1), 2 ** 32 - 1)


def gain_q12(db, lo=0, hi=capi.OVERLAY_G_MAX):
    """an amplitude gain in dB in Q12, clamped to [lo, hi]: [0, 32768] for the row laid over, [1, 65535] for a row's volume"""
    return min(max(int(round(4096 * 10 ** (db / 20))), lo), hi)


class Overlay:
    """one row of GpuDecoder.crop_overlay: source row a, with source row b (None: nothing) laid over it - at snr_db, the ratio of a's
    power to b's in dB, or at gain_db, b's own gain in dB; exactly one of the two with b - and the sum scaled by vol_db"""

    def __init__(self, a, b=None, snr_db=None, gain_db=None, vol_db=0.0):
        if b is None and (snr_db is not None or gain_db is not None):
            raise ValueError("Overlay: snr_db and gain_db belong to b")
        if b is not None and (snr_db is None) == (gain_db is None):
            raise ValueError("Overlay: exactly one of snr_db and gain_db with b")
        self.a, self.b, self.snr_db, self.gain_db, self.vol_db = a, b, snr_db, gain_db, vol_db
        # (a, b, vol, snr, gain) as acm_overlay_row holds them: made once, here, so that a call over many rows converts nothing
        self.raw = (a, capi.OVERLAY_NONE if b is None else b, gain_q12(vol_db, 1, 65535), snr_q16(snr_db) if snr_db is not None else 0,
                    gain_q12(gain_db) if gain_db is not None else 0)

    def record(self):
        """(a, b, vol, snr, gain) of acm_overlay_row, b None where nothing is laid over the row"""
        return (self.raw[0], self.b) + self.raw[2:]


class Response:
    """one impulse response of GpuDecoder.crop_overlay(responses=): h, a float array, quantised to what acm_fir_response holds -
    int16 taps q = nearbyint(h * 2^s) (float64, ties to even) with the largest shift s <= 30 at which max |q| <= 32767 and
    sum |q| <= 65535, so that a 32-bit accumulator is exact.  delay: the tap that lands on the input's own position - the direct
    path -, argmax |h| by default.  ValueError where no s >= 0 fits (sum |h| beyond 65535)."""

    def __init__(self, h, delay=None):
        h = np.asarray(h, dtype=np.float64).reshape(-1)
        if h.size == 0 or h.size > capi.FIR_MAX_TAPS or not np.isfinite(h).all():
            raise ValueError("Response: 1 .. %d finite taps" % capi.FIR_MAX_TAPS)
        delay = int(np.argmax(np.abs(h))) if delay is None else int(delay)
        for s in range(capi.FIR_MAX_SHIFT, -1, -1):
            q = np.rint(h * 2.0 ** s)
            if np.abs(q).max() <= 32767 and np.abs(q).sum() <= capi.FIR_MAX_L1:
                break
        else:
            raise ValueError("Response: sum |h| = %g does not fit %d at any shift" % (np.abs(h).sum(), capi.FIR_MAX_L1))
        self._set(q.astype(np.int16), delay, s)

    def _set(self, taps, delay, shift):
        if not 0 <= delay < taps.size:
            raise ValueError("Response: delay %d of %d taps" % (delay, taps.size))
        self.taps, self.delay, self.shift = taps, delay, shift
        self.record = (taps, delay, shift)      # as capi.fir_opts takes them

    @classmethod
    def raw(cls, taps, delay, shift):
        """a Response of integers as they are: int16 taps, delay, shift - what acm_dense_fir_check does not take is a ValueError"""
        r = cls.__new__(cls)
        t = np.asarray(taps)
        if t.ndim != 1 or t.size == 0 or (t != np.clip(np.rint(t), -32768, 32767)).any():
            raise ValueError("Response.raw: int16 taps")
        r._set(t.astype(np.int16), int(delay), int(shift))
        if capi.dense_fir_check(r.taps, r.delay, r.shift) != 0:
            raise ValueError("Response.raw: a response acm_dense_fir_check does not take")
        return r


def source_frames(frames, rate_in, rate_out, speed=(1, 1)):
    """the longest window, in frames of a file at rate_in played at speed = (num, den), whose crop fits a row of `frames` frames at
    rate_out (crop_batch(rate=rate_out, speed=...)): frames * M // L"""
    M, L = rate_in * speed[0], rate_out * speed[1]
    return frames * M // L


def _trace(trace, *ev):
    if trace is not None:
        trace.append(ev)


def decode_sharded(files, decoder, dist=None, root=0, device=None, chunks=1, ring=2, trace=None):
    """Decode `files` across all ranks of `dist`.

    `files`: list of paths (str / PathLike: every rank can open them; only `root` needs the list) and/or file images
    (bytes: every rank must pass the same list - contents are never sent, only ids).
    Returns on root: list of (status, np.uint16 array) in input order - np.float32 arrays where the decoder's `dtype` is torch.float32
    (GpuDecoder(dtype=torch.float32)); on other ranks: None.
    With dist=None runs single-process.  `decoder(list_of_bytes, out=None)` -> (pcm 1-D tensor of its dtype, offsets, words, statuses);
    a decoder without a `dtype` attribute is taken to produce int16.

    Order of communication, identical on every rank (RCCL runs the operations of one communicator in issue order):
        C1  scatter_object_list of the shard table (ids and paths)
        C1b gather_object of every rank's chunk plan: how many chunks, and the PCM capacity of each - known from headers and
            file lengths alone, so the root can post its receives before anything is decoded
        C2  point-to-point, pipelined: a rank decodes chunk k into one of TWO persistent buffers and sends it while chunk
            k + 1 decodes into the other (a buffer is reused once its send has completed); the root decodes its own chunks and
            meanwhile receives into a RING of `ring` buffers of one chunk each, copying every arrival to pinned host memory and
            posting the next receive into the freed slot - its HBM holds `ring` chunks of the others' PCM, not their shards
        C3  gather_object of the per-stream metadata (ids, offsets, words, statuses) once every transfer is done.
    `trace` (tests): a list that receives (event, ...) tuples in the order things happen on this rank.
    """
    import torch
    world = dist.get_world_size() if dist is not None else 1
    rank = dist.get_rank() if dist is not None else 0

    # ---- C1: shard table scatter (control): ids + paths, never contents
    if rank == root:
        weights = [file_weight(_head(f)) for f in files]
        shards = shard_longest_first(weights, world)
        table = [[(i, os.fspath(files[i]) if _is_path(files[i]) else None) for i in shard] for shard in shards]
    else:
        table = None
    if dist is not None:
        mine = [None]
        dist.scatter_object_list(mine, table if rank == root else None, src=root)
        mine = mine[0]
    else:
        mine = table[0]
    for i, path in mine:
        if path is None and (files is None or i >= len(files)):
            raise ValueError("decode_sharded: file %d was passed as bytes on the root only; pass paths, or the same list on every rank" % i)

    # ---- the chunk plan of this rank: whole files, capacities from headers + lengths
    nch = max(1, min(chunks, len(mine))) if mine else 0
    cuts = [len(mine) * k // nch for k in range(nch + 1)] if nch else [0]

    def capacity(i, path):
        if path is not None:
            return pcm_capacity_words(_head(path), os.path.getsize(path))
        return pcm_capacity_words(_head(files[i]), len(files[i]))
    caps = [sum(capacity(i, p) for i, p in mine[cuts[k]:cuts[k + 1]]) for k in range(nch)]

    # ---- C1b: every rank's chunk capacities to the root
    if dist is not None:
        all_caps = [None] * world if rank == root else None
        dist.gather_object(caps, all_caps, dst=root)
    else:
        all_caps = [caps]

    def decode_chunk(k, out):
        part = mine[cuts[k]:cuts[k + 1]]
        _trace(trace, "decode", k)
        pcm, offsets, words, statuses = decoder([_load(path if path is not None else files[i]) for i, path in part], out=out) \
            if out is not None else decoder([_load(path if path is not None else files[i]) for i, path in part])
        used = max([int(o) + int(w) for o, w in zip(offsets, words) if w] or [0])
        if used > caps[k]:
            raise RuntimeError("decode_sharded: chunk %d decoded %d words into a capacity of %d" % (k, used, caps[k]))
        meta = ([i for i, _ in part], [int(o) for o in offsets], [int(w) for w in words], [int(x) for x in statuses], used)
        return pcm, meta

    dtype = getattr(decoder, "dtype", torch.int16)      # of every PCM buffer here: the decoder's samples, int16 or float32

    def new_buffer(words, like=None):
        if hasattr(decoder, "empty"):
            return decoder.empty(words)
        return torch.empty(max(words, 1), dtype=dtype, device=device if device is not None else (like.device if like is not None else "cpu"))

    def to_host(t, words):
        """the first `words` of a PCM tensor as a host tensor (pinned + asynchronous for device memory)"""
        if t.is_cuda:
            h = torch.empty(max(words, 1), dtype=dtype, pin_memory=True)
            h[:words].copy_(t[:words], non_blocking=True)
            return h
        return t[:words].clone()

    # ---- a rank that is not the root: decode chunk k, send it, decode chunk k + 1 meanwhile
    if dist is not None and rank != root:
        bufs = [new_buffer(max(caps) if caps else 1), new_buffer(max(caps) if caps else 1)] if nch else []
        inflight = [None, None]
        metas = []
        for k in range(nch):
            b = k % 2
            if inflight[b] is not None:
                inflight[b].wait()              # this buffer's previous chunk has left
                _trace(trace, "send_done", k - 2)
            pcm, meta = decode_chunk(k, bufs[b] if hasattr(decoder, "empty") else None)
            if pcm.data_ptr() != bufs[b].data_ptr():
                bufs[b][:meta[4]].copy_(pcm[:meta[4]])          # a decoder with buffers of its own (the CPU stand-ins of the tests)
            metas.append(meta)
            if caps[k]:
                # neither RCCL nor gloo moves int16; bytes are bytes.  The chunk's capacity, not what was used: the root posted
                # its receive before this chunk was decoded
                inflight[b] = dist.isend(bufs[b][:caps[k]].view(torch.uint8), dst=root)
                _trace(trace, "send", k)
        for b, q in enumerate(inflight):
            if q is not None:
                q.wait()
        dist.gather_object(metas, None, dst=root)
        return None

    # ---- the root (or the only process): its own chunks, and meanwhile the ring of receives
    pending = [(r, k, all_caps[r][k]) for k in range(max([len(c) for c in all_caps] or [0]))
               for r in range(world) if r != root and k < len(all_caps[r]) and all_caps[r][k]]
    ring_words = max([c for _, _, c in pending] or [0])
    slots = [new_buffer(ring_words) for _ in range(min(max(1, ring), len(pending)))] if pending else []
    free_slots = list(range(len(slots)))
    posted = []                         # (request, slot, rank, chunk, words) in posting order
    arrived = {}                        # (rank, chunk) -> host tensor
    nxt = 0

    def post_receives():
        nonlocal nxt
        while nxt < len(pending) and free_slots:
            r, k, words = pending[nxt]
            j = free_slots.pop(0)
            posted.append((dist.irecv(slots[j][:words].view(torch.uint8), src=r), j, r, k, words))
            _trace(trace, "recv_posted", r, k)
            nxt += 1

    def collect(block):
        """arrivals in posting order (a communicator completes them in that order): copy out, free the slot"""
        while posted and (block or posted[0][0].is_completed()):
            q, j, r, k, words = posted.pop(0)
            q.wait()
            arrived[(r, k)] = to_host(slots[j], words)
            if slots[j].is_cuda:
                torch.cuda.current_stream().synchronize()       # the slot is about to be written again
            _trace(trace, "recv_done", r, k)
            free_slots.append(j)
            post_receives()
            if block:
                break

    own = []
    for k in range(nch):
        post_receives()
        pcm, meta = decode_chunk(k, None)
        if device is None:
            device = pcm.device
        own.append((meta, to_host(pcm, meta[4])))
        collect(False)
    post_receives()
    while posted:
        collect(True)
    if dist is not None:
        metas = [None] * world
        dist.gather_object([m for m, _ in own], metas, dst=root)
    else:
        metas = [[m for m, _ in own]]
    if torch.cuda.is_available() and any(h.is_pinned() for _, h in own):
        torch.cuda.synchronize()
    out = [None] * len(files)
    for r in range(world):
        for k, (ids_r, offs_r, words_r, st_r, _) in enumerate(metas[r]):
            h = own[k][1] if r == root else arrived.get((r, k))
            if dtype == torch.float32:
                host = h.numpy() if h is not None else np.zeros(0, np.float32)
            else:
                host = h.numpy().view(np.uint16) if h is not None else np.zeros(0, np.uint16)
            for i, o, w, st in zip(ids_r, offs_r, words_r, st_r):
                out[i] = (st, host[o:o + w].copy())
    return out
