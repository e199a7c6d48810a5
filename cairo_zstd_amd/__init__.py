"""cairo_zstd_amd — MI355X-native zstd frame/block decoder with the frame_decoder API surface of
NethermindEth/cairo_zstd.

Python here is a thin mirror over the C ABI (include/cairo_zstd_amd.h, libcairo_zstd_amd.so):
  * Context / decode_batch* : many independent frames per launch (the GPU hot path)
  * FrameDecoder            : FrameDecoderTrait call for call (src/frame_decoder.cairo:107-335)
  * read_frame_header / read_block_header : stateless parsers
  * compress / compress_batch_host / Context.compress_batch_device : batched compression on the device (split=True: a large
    buffer on many workgroups, still one frame; fse_tables=True: per-block FSE tables for the sequences; fast=True: the fast
    level, 32 KiB blocks that stand alone, one wave each; records=True: the records level, one wave per buffer of at most 32 KiB;
    fast_split=True: the fast level's frames with the 128 KiB groups of one buffer on many workgroups; high=True: the high-ratio
    level, two match tables, repeat-offset matches and a lazy parse; high_split=True: that level with the segments of one buffer
    on many workgroups)
  * compress_batch_host_dict / Context.compress_batch_dict_device : the same with dictionaries (Context.set_compress_dictionaries;
    records=True: the records level with dictionaries)
  * train_dictionary / Context.train_dictionary_device : a zstd dictionary made from samples on the device
  * Context.seekable_pack_device / Context.seekable_open_device / decode_seekable : a batch of frames as one seekable stream (the
    frames back to back and a seek table), packed and opened on the device; pack_seekable / open_seekable: the same on the CPU
  * Context.seekable_index / SeekableIndex.locate / Context.seekable_gather_device / read_seekable : byte ranges of such a stream's
    content, decoding only the frames they touch; locate_seekable: the locate on the CPU
All decoding and compression runs in the HIP kernels; nothing here decodes or compresses on the CPU.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import status
from ._lib import (COMPRESS_CHECKSUM, COMPRESS_FAST, COMPRESS_FAST_SPLIT, COMPRESS_HIGH, COMPRESS_HIGH_SPLIT, COMPRESS_RECORDS, COMPRESS_FSE_TABLES, COMPRESS_NO_DICT, COMPRESS_NO_DICT_ID, COMPRESS_RESULT_DTYPE, COMPRESS_SPLIT, SEEKABLE_CHECKSUMS, SEEKABLE_INFO_DTYPE, SEEKABLE_READ_INFO_DTYPE, SEEKABLE_SPAN_DTYPE, TRAIN_MIN_CAPACITY, RESULT_CHECKSUM_COMPUTED, RESULT_CHECKSUM_MATCH, RESULT_DTYPE, RESULT_FINISHED, RESULT_HAS_CHECKSUM,
                   BlockHeader, FrameHeader, build, lib)

DEBUG_CHAIN_CPP_STEP, DEBUG_NO_HUF1, DEBUG_WX_POISON, DEBUG_EXEC_FIRST, DEBUG_EXEC_LEAVE = 1, 2, 4, 8, 16     # cz_context_set_debug_flags
from .status import CzError

__all__ = ["Context", "FrameDecoder", "BlockDecodingStrategy", "decode_batch_host", "read_frame_header",
           "read_block_header", "graph_replay_available", "RESULT_DTYPE", "RESULT_FINISHED", "RESULT_HAS_CHECKSUM", "RESULT_CHECKSUM_COMPUTED",
           "RESULT_CHECKSUM_MATCH", "status", "CzError", "build", "lib", "compress_bound", "compress_batch_host", "compress",
           "COMPRESS_CHECKSUM", "COMPRESS_RESULT_DTYPE", "compress_batch_host_dict", "COMPRESS_NO_DICT", "COMPRESS_NO_DICT_ID",
           "COMPRESS_SPLIT", "compress_split_segment", "COMPRESS_FSE_TABLES", "COMPRESS_FAST", "COMPRESS_FAST_SPLIT", "COMPRESS_HIGH", "COMPRESS_HIGH_SPLIT", "COMPRESS_RECORDS", "compress_record_max", "train_dictionary", "TRAIN_MIN_CAPACITY",
           "SEEKABLE_CHECKSUMS", "SEEKABLE_INFO_DTYPE", "seekable_bound", "pack_seekable", "open_seekable", "decode_seekable",
           "SEEKABLE_READ_INFO_DTYPE", "SEEKABLE_SPAN_DTYPE", "SeekableIndex", "locate_seekable", "read_seekable"]


def _as_u8(b) -> np.ndarray:
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, dtype=np.uint8)
    return np.frombuffer(bytes(b), dtype=np.uint8)


def graph_replay_available() -> bool:
    """cz_graph_replay_available: whether a repeated launch can be captured as a hipGraph in this process (Context.set_graph_replay)."""
    return bool(lib().cz_graph_replay_available())


class Context:
    """Device context (cz_context_*).  `stream` is a raw hipStream_t (e.g.
    torch.cuda.current_stream().cuda_stream) or None for a private stream."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._h = C.c_void_p()
        st = lib().cz_context_create(C.byref(self._h), device, C.c_void_p(stream) if stream else None)
        if st:
            self._h = None
            raise CzError(st, "cz_context_create")
        self.device = device
        self._decoders = weakref.WeakSet()

    def close(self):
        if getattr(self, "_h", None):
            for fd in list(self._decoders):      # frame decoders and seekable indexes hold device memory of this context
                fd.close()
            lib().cz_context_destroy(self._h)
            self._h = None

    __del__ = close

    def synchronize(self):
        st = lib().cz_context_synchronize(self._h)
        if st:
            raise CzError(st, f"hip error {lib().cz_context_last_hip_error(self._h)}")

    def launch_info(self):
        wg, th, cu = C.c_int(), C.c_int(), C.c_int()
        lib().cz_context_launch_info(self._h, C.byref(wg), C.byref(th), C.byref(cu))
        return dict(workgroups=wg.value, threads_per_workgroup=th.value, compute_units=cu.value)

    def execute_grid(self):
        """(waves of cz_execute_frames_kernel, waves of its 8-waves build) a batch launch runs with."""
        a, b = C.c_int(), C.c_int()
        lib().cz_context_execute_grid(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def set_chain_arena(self, nbytes: int, min_sequences: int | None = None):
        """Enable (nbytes > 0) / disable (0) the FSE-chain pre-pass (cz_chain_kernel) for batch decodes."""
        if min_sequences is not None:
            lib().cz_context_set_chain_min_sequences(self._h, min_sequences)
        st = lib().cz_context_set_chain_arena(self._h, nbytes)
        if st:
            raise CzError(st, f"hip error {lib().cz_context_last_hip_error(self._h)}")

    def set_verify_checksum(self, on: bool = True):
        """Compute and compare the XXH64 content checksum of every checksummed frame on the device."""
        lib().cz_context_set_verify_checksum(self._h, 1 if on else 0)
        self._verify = bool(on)

    def set_dictionary(self, dictionary: "Dictionary | None"):
        """Batch decodes start every frame from `dictionary` (None: from nothing): init_from_dict, src/decoding/scratch.cairo:60-65."""
        self._dict = dictionary
        st = lib().cz_context_set_dictionary(self._h, dictionary._h if dictionary is not None else None)
        if st:
            raise CzError(st, "cz_context_set_dictionary")

    def set_dictionaries(self, dicts, no_id: "Dictionary | None" = None):
        """Batch decodes pick each frame's dictionary by the Dictionary_ID of its header: the one of `dicts` with that ID, `no_id`
        for frames without an ID (None: no dictionary); any other ID fails the frame with CZ_E_DICT_UNKNOWN (detail[0] = the ID).
        An empty `dicts` with no `no_id` clears the setting.  Replaces set_dictionary's setting and is replaced by it."""
        dicts = list(dicts)
        arr = (C.c_void_p * max(len(dicts), 1))(*[d._h if d is not None else None for d in dicts])
        st = lib().cz_context_set_dictionaries(self._h, arr if dicts else None, len(dicts), no_id._h if no_id is not None else None)
        if st:
            raise CzError(st, "cz_context_set_dictionaries")
        self._dict = (dicts, no_id)                                      # keep them alive while launches use them

    def set_compress_dictionaries(self, dicts):
        """The dictionaries later compress_batch_dict_* calls pick from by index (cz_context_set_compress_dictionaries); an empty
        list clears the setting.  Independent of set_dictionary / set_dictionaries."""
        dicts = list(dicts)
        arr = (C.c_void_p * max(len(dicts), 1))(*[d._h if d is not None else None for d in dicts])
        st = lib().cz_context_set_compress_dictionaries(self._h, arr if dicts else None, len(dicts))
        if st:
            raise CzError(st, "cz_context_set_compress_dictionaries")
        self._cdict = dicts                                              # keep them alive while launches use them

    def last_chain_ms(self) -> float:
        """Milliseconds of the last launch spent in the FSE-chain pre-pass kernel (0 when it is off)."""
        ms = C.c_float(0)
        st = lib().cz_context_last_chain_ms(self._h, C.byref(ms))
        if st:
            raise CzError(st, "cz_context_last_chain_ms")
        return float(ms.value)

    def set_literal_arena(self, nbytes: int):
        """Enable (nbytes > 0) / disable (0) the block-parallel huff0 / tile kernels and the execute-only frame kernel (cz_context_set_literal_arena)."""
        st = lib().cz_context_set_literal_arena(self._h, nbytes)
        if st:
            raise CzError(st, f"hip error {lib().cz_context_last_hip_error(self._h)}")

    def last_prepass_counts(self, n: int):
        """(frames with chain records, frames with literal nodes) of the last batch launch of n frames."""
        a, b = C.c_size_t(), C.c_size_t()
        lib().cz_context_last_prepass_counts(self._h, n, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def last_literals_tail_ms(self) -> float:
        """Milliseconds the last launch went on with the huff0 / tile kernels after the chain kernel was done."""
        ms = C.c_float(0)
        lib().cz_context_last_literals_tail_ms(self._h, C.byref(ms))
        return float(ms.value)

    def set_exec_kernel(self, on: bool = True):
        """Frames the pre-pass finished (chain records and literals) run on cz_execute_frames_kernel (default); off: like every
        other frame, on cz_decode_frames_kernel."""
        lib().cz_context_set_exec_kernel(self._h, 1 if on else 0)

    def set_wexec_kernel(self, on: bool = True, cus: int = 0, leave_per_cu: int = 0, force: bool = False):
        """cz_wexec_kernel (a workgroup per frame, the block in hand in an LDS window) side by side with cz_execute_frames_kernel on
        batches whose far offsets outweigh the near ones (decided on the device; default on).  cus / leave_per_cu / force: the A/B
        knobs of cz_context_set_wexec_tuning (force: side by side whatever the offsets look like)."""
        lib().cz_context_set_wexec_kernel(self._h, 1 if on else 0)
        st = lib().cz_context_set_wexec_tuning(self._h, int(cus), int(leave_per_cu), int(force))
        if st:
            raise CzError(st, "cz_context_set_wexec_tuning")

    def measure_batch(self, d_in_base: int, d_in_off: int, d_in_len: int, n: int, d_out_cap: int):
        """(chain arena bytes, literal arena bytes) a batch on the device needs, from its headers (cz_context_measure_batch)."""
        a, b = C.c_size_t(), C.c_size_t()
        st = lib().cz_context_measure_batch(self._h, d_in_base, d_in_off, d_in_len, n, d_out_cap, C.byref(a), C.byref(b))
        if st:
            raise CzError(st, "cz_context_measure_batch")
        return int(a.value), int(b.value)

    def set_debug_flags(self, flags: int):
        """Test knobs (cz_context_set_debug_flags): DEBUG_CHAIN_CPP_STEP, DEBUG_NO_HUF1, DEBUG_WX_POISON, DEBUG_EXEC_FIRST, DEBUG_EXEC_LEAVE."""
        lib().cz_context_set_debug_flags(self._h, int(flags))

    def debug_read_chain_arena(self, nbytes: int):
        """(first nbytes of the chain arena as a uint64 array, arena units in use) after the last launch."""
        import numpy as _np
        buf = _np.zeros(nbytes // 8, dtype=_np.uint64)
        used = C.c_uint64(0)
        st = lib().cz_context_debug_read_chain_arena(self._h, buf.ctypes.data, buf.nbytes, C.byref(used))
        if st:
            raise CzError(st, "cz_context_debug_read_chain_arena")
        return buf, int(used.value)

    def last_sequence_stats(self):
        """(near-offset, far-offset, long-run) sequence sums of the last launch (x 4), as cz_chain_kernel took them from the code tables."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        lib().cz_context_last_sequence_stats(self._h, C.byref(a), C.byref(b), C.byref(c))
        return int(a.value), int(b.value), int(c.value)

    def set_early_execute(self, on: bool):
        """Two chain launches (large blocks / all others) with the early execute launches behind the second, or one (default)."""
        lib().cz_context_set_early_execute(self._h, 1 if on else 0)

    def set_graph_replay(self, on: bool):
        """on: a launch that repeats the one before it is captured as a hipGraph and replayed from then on, where
        graph_replay_available(); off (default): never."""
        lib().cz_context_set_graph_replay(self._h, 1 if on else 0)

    def last_launch_was_replay(self) -> bool:
        """Whether the last batch launch was the replay of a captured graph."""
        return bool(lib().cz_context_last_launch_was_replay(self._h))

    def last_small_ms(self) -> float:
        """When the small blocks' chains and all literals of the last launch were done, ms from its start (0: not a split launch)."""
        ms = C.c_float(0)
        lib().cz_context_last_small_ms(self._h, C.byref(ms))
        return float(ms.value)

    def last_fallback_count(self) -> int:
        """Frames the pre-pass and execute kernels of the last launch handed to cz_decode_frames_kernel (each listed once)."""
        a = C.c_size_t()
        lib().cz_context_last_fallback_count(self._h, C.byref(a))
        return int(a.value)

    def last_wexec_counts(self):
        """(frames listed for cz_wexec_kernel, frames it finished, frames it handed on) in the last launch."""
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        lib().cz_context_last_wexec_counts(self._h, C.byref(a), C.byref(b), C.byref(c))
        return int(a.value), int(b.value), int(c.value)

    def last_side_counts(self):
        """(workgroups of cz_wexec_kernel that counted themselves in, waves of cz_execute_frames_kernel that left the CUs to it, waves
        that waited for it and stayed) in the last launch, side by side."""
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        st = lib().cz_context_last_side_counts(self._h, C.byref(a), C.byref(b), C.byref(c))
        if st:
            raise CzError(st, "cz_context_last_side_counts")
        return int(a.value), int(b.value), int(c.value)

    def last_wexec_ms(self) -> float:
        """Milliseconds of the last launch spent in cz_wexec_kernel (0 when it did not run)."""
        ms = C.c_float(0)
        st = lib().cz_context_last_wexec_ms(self._h, C.byref(ms))
        if st:
            raise CzError(st, "cz_context_last_wexec_ms")
        return float(ms.value)

    def last_exec_ms(self) -> float:
        """Milliseconds of the last launch spent in cz_execute_frames_kernel (0 when it did not run)."""
        ms = C.c_float(0)
        st = lib().cz_context_last_exec_ms(self._h, C.byref(ms))
        if st:
            raise CzError(st, "cz_context_last_exec_ms")
        return float(ms.value)

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        st = lib().cz_context_last_kernel_ms(self._h, C.byref(ms))
        if st:
            raise CzError(st, "cz_context_last_kernel_ms")
        return ms.value

    def decode_batch_device(self, in_base: int, in_off: int, in_len: int, n: int, out_base: int, out_off: int,
                            out_cap: int, results: int):
        """All arguments are raw DEVICE pointers (tensor.data_ptr()).  Asynchronous on the context's stream — which is a stream of
        the context's own when it was created with handle 0 (torch's default stream): synchronise between torch's writes to these
        buffers and this call, and before reading the results."""
        st = lib().cz_decode_batch_device(self._h, in_base, in_off, in_len, n, out_base, out_off, out_cap, results)
        if st:
            raise CzError(st, f"hip error {lib().cz_context_last_hip_error(self._h)}")

    def decode_batch_host(self, in_base, in_off, in_len, out_off, out_cap, out_total: int):
        """Host buffers in, host buffers out (PCIe-inclusive).  Returns (out_base, results)."""
        in_base = _as_u8(in_base)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint64)
        out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
        out_cap = np.ascontiguousarray(out_cap, dtype=np.uint64)
        n = int(in_off.size)
        out = np.zeros(max(out_total, 1), dtype=np.uint8)
        res = np.zeros(n, dtype=RESULT_DTYPE)
        st = lib().cz_decode_batch_host(self._h, in_base.ctypes.data, in_base.size, in_off.ctypes.data, in_len.ctypes.data,
                                        n, out.ctypes.data, out_total, out_off.ctypes.data, out_cap.ctypes.data,
                                        res.ctypes.data)
        if st:
            raise CzError(st, f"hip error {lib().cz_context_last_hip_error(self._h)}")
        return out, res

    def compress_batch_device(self, in_base: int, in_off: int, in_len: int, n: int, out_base: int, out_off: int,
                              out_cap: int, results: int, checksum: bool = False, split: bool = False, fse_tables: bool = False,
                              fast: bool = False, records: bool = False, fast_split: bool = False, high: bool = False,
                              high_split: bool = False):
        """cz_compress_batch_device.  All arguments are raw DEVICE pointers (tensor.data_ptr()); `results` holds n
        COMPRESS_RESULT_DTYPE records.  Asynchronous on the context's stream, like decode_batch_device.  split=True
        (COMPRESS_SPLIT): inputs longer than compress_split_segment() are compressed by several workgroups, still one frame each.
        fse_tables=True (COMPRESS_FSE_TABLES): each block's sequences take tables of its own where they make it smaller.
        fast=True (COMPRESS_FAST): the fast level, 32 KiB blocks that stand alone; not with split or fse_tables.
        records=True (COMPRESS_RECORDS): the records level, one wave per input of at most compress_record_max() bytes; not with
        split, fse_tables or fast.
        fast_split=True (COMPRESS_FAST_SPLIT): the fast level's frames, byte for byte, with the 128 KiB groups of one input on many
        workgroups; with checksum alone.
        high=True (COMPRESS_HIGH): the high-ratio level, the COMPRESS_FSE_TABLES frame with better sequences; with checksum alone.
        high_split=True (COMPRESS_HIGH_SPLIT): the high-ratio level with the segments of one input (compress_split_segment() bytes
        each) on many workgroups, still one frame each; with checksum alone."""
        st = lib().cz_compress_batch_device(self._h, in_base, in_off, in_len, n, out_base, out_off, out_cap,
                                            _compress_flags(checksum, split, fse_tables, fast, records, fast_split, high, high_split), results)
        if st:
            raise CzError(st, f"hip error {lib().cz_context_last_hip_error(self._h)}")

    def compress_batch_host(self, in_base, in_off, in_len, out_off, out_cap, out: np.ndarray, checksum: bool = False,
                            split: bool = False, fse_tables: bool = False, fast: bool = False, records: bool = False,
                            fast_split: bool = False, high: bool = False, high_split: bool = False):
        """cz_compress_batch_host: host buffers in, `out` (uint8, written in place) out.  Returns the result records."""
        in_base = _as_u8(in_base)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint64)
        out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
        out_cap = np.ascontiguousarray(out_cap, dtype=np.uint64)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
        n = int(in_off.size)
        res = np.zeros(n, dtype=COMPRESS_RESULT_DTYPE)
        st = lib().cz_compress_batch_host(self._h, in_base.ctypes.data if in_base.size else None, in_base.size, in_off.ctypes.data,
                                          in_len.ctypes.data, n, out.ctypes.data, out.size, out_off.ctypes.data, out_cap.ctypes.data,
                                          _compress_flags(checksum, split, fse_tables, fast, records, fast_split, high, high_split), res.ctypes.data)
        if st:
            raise CzError(st, f"hip error {lib().cz_context_last_hip_error(self._h)}")
        return res

    def compress_batch_dict_device(self, in_base: int, in_off: int, in_len: int, n: int, out_base: int, out_off: int,
                                   out_cap: int, dict_index: int, results: int, checksum: bool = False, dict_id: bool = True,
                                   records: bool = False, fast_split: bool = False, high_split: bool = False):
        """cz_compress_batch_dict_device: as compress_batch_device, frame i with dictionary dict_index[i] of
        set_compress_dictionaries (COMPRESS_NO_DICT: none).  dict_index is a DEVICE pointer to n uint32 (0: every frame uses the
        one dictionary set).  dict_id=False omits the Dictionary_ID field.  records=True (COMPRESS_RECORDS): the records level.
        fast_split=True (COMPRESS_FAST_SPLIT) and high_split=True (COMPRESS_HIGH_SPLIT) are refused here, as by the library: those
        levels take no dictionary."""
        flags = ((COMPRESS_CHECKSUM if checksum else 0) | (0 if dict_id else COMPRESS_NO_DICT_ID) | (COMPRESS_RECORDS if records else 0)
                 | (COMPRESS_FAST_SPLIT if fast_split else 0) | (COMPRESS_HIGH_SPLIT if high_split else 0))
        st = lib().cz_compress_batch_dict_device(self._h, in_base, in_off, in_len, n, out_base, out_off, out_cap, flags,
                                                 dict_index or None, results)
        if st:
            raise CzError(st, f"hip error {lib().cz_context_last_hip_error(self._h)}")

    def compress_batch_dict_host(self, in_base, in_off, in_len, out_off, out_cap, out: np.ndarray, dict_index,
                                 checksum: bool = False, dict_id: bool = True, records: bool = False, fast_split: bool = False,
                                 high_split: bool = False):
        """cz_compress_batch_dict_host: as compress_batch_host, with a dictionary index per buffer (None: every buffer uses the
        one dictionary set).  records=True (COMPRESS_RECORDS): the records level.  fast_split=True and high_split=True are refused, as by the library.
        Returns the result records."""
        in_base = _as_u8(in_base)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        in_len = np.ascontiguousarray(in_len, dtype=np.uint64)
        out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
        out_cap = np.ascontiguousarray(out_cap, dtype=np.uint64)
        idx = None if dict_index is None else np.ascontiguousarray(dict_index, dtype=np.uint32)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
        n = int(in_off.size)
        res = np.zeros(n, dtype=COMPRESS_RESULT_DTYPE)
        flags = ((COMPRESS_CHECKSUM if checksum else 0) | (0 if dict_id else COMPRESS_NO_DICT_ID) | (COMPRESS_RECORDS if records else 0)
                 | (COMPRESS_FAST_SPLIT if fast_split else 0) | (COMPRESS_HIGH_SPLIT if high_split else 0))
        st = lib().cz_compress_batch_dict_host(self._h, in_base.ctypes.data if in_base.size else None, in_base.size, in_off.ctypes.data,
                                               in_len.ctypes.data, n, out.ctypes.data, out.size, out_off.ctypes.data, out_cap.ctypes.data,
                                               flags, None if idx is None else idx.ctypes.data, res.ctypes.data)
        if st:
            raise CzError(st, f"hip error {lib().cz_context_last_hip_error(self._h)}")
        return res

    def train_dictionary_device(self, base: int, off: int, length: int, n: int, d_dict: int, capacity: int, dict_id: int = 0,
                                segment_len: int = 0) -> int:
        """cz_dictionary_train_device: a zstd dictionary from n samples in HBM (raw device pointers: base, off[] and len[] as uint64)
        into the capacity bytes at d_dict.  Returns the dictionary's length.  Synchronises."""
        params = (C.c_uint32 * 8)(dict_id, segment_len)
        got = C.c_size_t(0)
        st = lib().cz_dictionary_train_device(self._h, base, off, length, n, d_dict, capacity, params, C.byref(got))
        if st:
            raise CzError(st, f"cz_dictionary_train_device (hip error {lib().cz_context_last_hip_error(self._h)})")
        return int(got.value)

    def train_dictionary_host(self, base, off, length, capacity: int, dict_id: int = 0, segment_len: int = 0, fill: int = 0):
        """cz_dictionary_train_host: the same from host arrays.  Returns (the whole capacity-byte buffer, pre-set to `fill`; the
        dictionary's length)."""
        base = _as_u8(base)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint64)
        out = np.full(max(int(capacity), 1), fill, dtype=np.uint8)
        params = (C.c_uint32 * 8)(dict_id, segment_len)
        got = C.c_size_t(0)
        st = lib().cz_dictionary_train_host(self._h, base.ctypes.data if base.size else None, base.size, off.ctypes.data, length.ctypes.data,
                                            int(off.size), out.ctypes.data, capacity, params, C.byref(got))
        if st:
            raise CzError(st, f"cz_dictionary_train_host (hip error {lib().cz_context_last_hip_error(self._h)})")
        return out, int(got.value)

    def seekable_pack_device(self, frames_base: int, frame_off: int, results: int, n: int, stream: int, stream_cap: int, info: int,
                             checksums: bool = False):
        """cz_seekable_pack_device: the n frames a compress_batch_*device call left at frames_base + frame_off[i] (their lengths and
        sizes in `results`) back to back into `stream`, followed by the seek table.  All arguments are raw DEVICE pointers, `info`
        (one SEEKABLE_INFO_DTYPE record, which carries the status of everything decided on the device) included.  Asynchronous on
        the context's stream and never synchronises: directly behind the compress launch it needs no host step in between."""
        st = lib().cz_seekable_pack_device(self._h, frames_base or None, frame_off or None, results or None, n, stream, stream_cap,
                                           SEEKABLE_CHECKSUMS if checksums else 0, info)
        if st:
            raise CzError(st, f"cz_seekable_pack_device (hip error {lib().cz_context_last_hip_error(self._h)})")

    def seekable_open_device(self, stream: int, stream_len: int, first: int = 0, count: int | None = None, out_align: int = 1,
                             in_off: int = 0, in_len: int = 0, out_off: int = 0, out_cap: int = 0, checksum: int = 0):
        """cz_seekable_open_device: validates the seek table of the stream at the DEVICE pointer `stream` and writes the arrays of
        decode_batch_device for frames [first, first + count) (count None: up to the end) to the DEVICE pointers given (0: not
        wanted; all 0: the sizing call).  Synchronises.  Returns the SEEKABLE_INFO_DTYPE record: status (CZ_OK, CZ_E_SEEK_TABLE with
        its reason, CZ_E_INVALID_ARG), the table's sums, and in `detail` the output bytes the range needs."""
        info = np.zeros(1, dtype=SEEKABLE_INFO_DTYPE)
        st = lib().cz_seekable_open_device(self._h, stream or None, stream_len, first, 0xFFFFFFFFFFFFFFFF if count is None else count, out_align,
                                           in_off or None, in_len or None, out_off or None, out_cap or None, checksum or None, info.ctypes.data)
        if st == status.CZ_E_HIP:
            raise CzError(st, f"cz_seekable_open_device (hip error {lib().cz_context_last_hip_error(self._h)})")
        return info[0]

    def seekable_index(self, stream: int, stream_len: int) -> "SeekableIndex":
        """cz_seekable_index_create_device: the index of the stream at the DEVICE pointer `stream` (its table validated as by
        seekable_open_device; the scans of its sizes and its checksums kept in HBM).  Synchronises; the stream need not outlive the
        call.  Raises CzError on a malformed table (with the reason)."""
        return SeekableIndex(self, stream, stream_len)

    def seekable_gather_device(self, decoded: int, out_off: int, content_off: int, k: int, range_off: int, range_len: int, spans: int,
                               m: int, dst: int, dst_bytes: int):
        """cz_seekable_gather_device: the m ranges out of the k decoded frames of one SeekableIndex.locate (its arrays, as raw DEVICE
        pointers) back to back into `dst`.  Asynchronous on the context's stream and never synchronises: directly behind the
        decode launch it needs no host step in between."""
        st = lib().cz_seekable_gather_device(self._h, decoded or None, out_off or None, content_off or None, k, range_off or None,
                                             range_len or None, spans or None, m, dst or None, dst_bytes)
        if st:
            raise CzError(st, f"cz_seekable_gather_device (hip error {lib().cz_context_last_hip_error(self._h)})")

    def last_train_ms(self):
        """cz_dictionary_train_last_ms: device milliseconds of the last training's steps (frequencies, epochs, statistics, tables)."""
        ms = (C.c_float * 4)()
        st = lib().cz_dictionary_train_last_ms(self._h, ms)
        if st:
            raise CzError(st, "cz_dictionary_train_last_ms")
        return [float(x) for x in ms]


def train_dictionary(samples, capacity: int, ctx: Context, dict_id: int = 0, segment_len: int = 0) -> bytes:
    """A zstd dictionary of at most `capacity` bytes trained on the device from `samples` (a list of buffers): content chosen by
    d-mer coverage, entropy tables from parsing the samples against it.  dict_id 0: derived from the content; segment_len 0: 128."""
    lens = np.array([len(b) for b in samples], dtype=np.uint64)
    off = np.zeros(len(samples), dtype=np.uint64)
    if len(samples) > 1:
        off[1:] = np.cumsum(lens[:-1])
    base = np.frombuffer(b"".join(bytes(b) for b in samples) + b"\0" * 16, dtype=np.uint8)
    out, n = ctx.train_dictionary_host(base, off, lens, capacity, dict_id=dict_id, segment_len=segment_len)
    return out[:n].tobytes()


def seekable_bound(frame_bytes: int, n: int, checksums: bool = False) -> int:
    """cz_seekable_bound: the bytes of the seekable stream of n frames of frame_bytes bytes together."""
    return int(lib().cz_seekable_bound(frame_bytes, n, SEEKABLE_CHECKSUMS if checksums else 0))


def pack_seekable(frames, content_sizes, checksums=None) -> bytes:
    """cz_seekable_pack_host (on the CPU, no device): the frames back to back and the seek table with their lengths, content_sizes
    and, when given, checksums (the low 32 bits of XXH64 of each frame's content)."""
    n = len(frames)
    res = np.zeros(max(n, 1), dtype=COMPRESS_RESULT_DTYPE)
    lens = np.array([len(f) for f in frames], dtype=np.uint64)
    res["bytes_written"][:n] = lens
    res["bytes_read"][:n] = np.asarray(content_sizes, dtype=np.uint64)
    if checksums is not None:
        res["checksum"][:n] = np.asarray(checksums, dtype=np.uint32)
        res["flags"][:n] = COMPRESS_CHECKSUM
    off = np.zeros(max(n, 1), dtype=np.uint64)
    off[1:n] = np.cumsum(lens[:-1])
    base = np.frombuffer(b"".join(bytes(f) for f in frames) + b"\0", dtype=np.uint8)
    cap = seekable_bound(int(lens.sum()), n, checksums is not None)
    out = np.zeros(cap, dtype=np.uint8)
    info = np.zeros(1, dtype=SEEKABLE_INFO_DTYPE)
    st = lib().cz_seekable_pack_host(base.ctypes.data, off.ctypes.data, res.ctypes.data, n, out.ctypes.data, cap,
                                     SEEKABLE_CHECKSUMS if checksums is not None else 0, info.ctypes.data)
    if st:
        raise CzError(st, f"cz_seekable_pack_host (frame {int(info[0]['detail'])})")
    return out[:int(info[0]["stream_bytes"])].tobytes()


def open_seekable(stream, first: int = 0, count: int | None = None, out_align: int = 1):
    """cz_seekable_open_host (on the CPU, no device): (info, in_off, in_len, out_off, out_cap, checksums) of frames
    [first, first + count) of a seekable stream (count None: up to the end), the arrays as decode_batch_* take them.  `info` is the
    SEEKABLE_INFO_DTYPE record; when its status is not CZ_OK (CZ_E_SEEK_TABLE with the reason, CZ_E_INVALID_ARG) the arrays are empty."""
    a = _as_u8(stream)
    info = np.zeros(1, dtype=SEEKABLE_INFO_DTYPE)
    none = 0xFFFFFFFFFFFFFFFF
    st = lib().cz_seekable_open_host(a.ctypes.data if a.size else None, a.size, first, none if count is None else count, out_align,
                                     None, None, None, None, None, info.ctypes.data)
    k = 0
    if not st:
        k = int(info[0]["frames"]) - first if count is None else count
    arr = [np.zeros(k, dtype=np.uint64) for _ in range(4)] + [np.zeros(k, dtype=np.uint32)]
    if k:
        lib().cz_seekable_open_host(a.ctypes.data, a.size, first, k, out_align, *[x.ctypes.data for x in arr], info.ctypes.data)
    return (info[0], *arr)


def decode_seekable(stream, ctx: Context, first: int = 0, count: int | None = None):
    """Frames [first, first + count) of a seekable stream (count None: up to the end), decoded: a list of bytes.  The stream is
    staged in HBM, its table opened there (cz_seekable_open_device) and the range decoded by ONE decode_batch_device; nothing but
    the stream goes up and nothing but the decoded bytes and the result records come down.  Raises CzError on a malformed table,
    a range outside it, or a frame that fails."""
    import torch
    a = _as_u8(stream)
    dev = torch.device(f"cuda:{ctx.device}")
    d_stream = torch.zeros(a.size + 64, dtype=torch.uint8, device=dev)
    d_stream[:a.size] = torch.from_numpy(a.copy())
    torch.cuda.synchronize(dev)
    info = ctx.seekable_open_device(d_stream.data_ptr(), a.size, first, count, 256)
    if int(info["status"]):
        raise CzError(int(info["status"]), f"cz_seekable_open_device (reason {int(info['reason'])})")
    k = int(info["frames"]) - first if count is None else count
    if k == 0:
        return []
    desc = torch.zeros((4, k), dtype=torch.int64, device=dev)
    d_out = torch.zeros(int(info["detail"]) + 256, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(k * RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    info = ctx.seekable_open_device(d_stream.data_ptr(), a.size, first, k, 256, desc[0].data_ptr(), desc[1].data_ptr(), desc[2].data_ptr(),
                                    desc[3].data_ptr())
    if int(info["status"]):
        raise CzError(int(info["status"]), "cz_seekable_open_device")
    ctx.decode_batch_device(d_stream.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), k, d_out.data_ptr(), desc[2].data_ptr(),
                            desc[3].data_ptr(), d_res.data_ptr())
    ctx.synchronize()
    res = d_res.cpu().numpy().view(RESULT_DTYPE)
    out, off = d_out.cpu().numpy(), desc[2].cpu().numpy()
    for i in range(k):
        if int(res[i]["status"]):
            raise CzError(int(res[i]["status"]), f"frame {first + i}")
    return [out[int(off[i]): int(off[i]) + int(res[i]["bytes_produced"])].tobytes() for i in range(k)]


class SeekableIndex:
    """cz_seekable_index: a seekable stream's table, validated and scanned once, in HBM (Context.seekable_index).  `.info` is the
    SEEKABLE_INFO_DTYPE record of the table."""

    def __init__(self, ctx: Context, stream: int, stream_len: int):
        self._h = None
        info = np.zeros(1, dtype=SEEKABLE_INFO_DTYPE)
        h = C.c_void_p()
        st = lib().cz_seekable_index_create_device(ctx._h, stream or None, stream_len, C.byref(h), info.ctypes.data)
        if st == status.CZ_E_HIP:
            raise CzError(st, f"cz_seekable_index_create_device (hip error {lib().cz_context_last_hip_error(ctx._h)})")
        if st:
            raise CzError(st, f"cz_seekable_index_create_device (reason {int(info[0]['reason'])})")
        self._h, self.ctx, self.info = h, ctx, info[0]
        ctx._decoders.add(self)

    def locate(self, range_off: int, range_len: int, m: int, out_align: int = 1, frames_cap: int = 0, frame: int = 0, in_off: int = 0,
               in_len: int = 0, out_off: int = 0, out_cap: int = 0, checksum: int = 0, content_off: int = 0, spans: int = 0):
        """cz_seekable_locate_device: which frames hold a byte of the m ranges at the DEVICE pointers range_off / range_len, and
        where each range lies in their decode output.  The arrays go to the DEVICE pointers given (0: not wanted; all 0: the sizing
        call).  Synchronises.  Returns the SEEKABLE_READ_INFO_DTYPE record: status (CZ_OK; CZ_E_INVALID_ARG with the lowest index of
        a range outside the content in `detail`; CZ_E_OUTPUT_TOO_SMALL when more than frames_cap frames are selected), `selected`,
        `out_bytes` and `dst_bytes`."""
        info = np.zeros(1, dtype=SEEKABLE_READ_INFO_DTYPE)
        st = lib().cz_seekable_locate_device(self._h, range_off or None, range_len or None, m, out_align, frames_cap, frame or None,
                                             in_off or None, in_len or None, out_off or None, out_cap or None, checksum or None,
                                             content_off or None, spans or None, info.ctypes.data)
        if st == status.CZ_E_HIP:
            raise CzError(st, f"cz_seekable_locate_device (hip error {lib().cz_context_last_hip_error(self.ctx._h)})")
        return info[0]

    def close(self):
        if getattr(self, "_h", None):
            lib().cz_seekable_index_destroy(self._h)
            self._h = None

    __del__ = close


def locate_seekable(stream, ranges, out_align: int = 1):
    """cz_seekable_locate_host (on the CPU, no device): (info, frame, in_off, in_len, out_off, out_cap, checksums, content_off, spans)
    for `ranges`, a list of (offset, length) in the content of the seekable stream: the frames that hold a requested byte, as
    decode_batch_* take them, and per range a SEEKABLE_SPAN_DTYPE record.  `info` is the SEEKABLE_READ_INFO_DTYPE record; when its
    status is not CZ_OK (CZ_E_SEEK_TABLE with the reason, CZ_E_INVALID_ARG with the range in `detail`) the arrays are empty."""
    a = _as_u8(stream)
    m = len(ranges)
    r = np.array(ranges, dtype=np.uint64).reshape(m, 2)
    off, ln = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
    info = np.zeros(1, dtype=SEEKABLE_READ_INFO_DTYPE)
    args = (a.ctypes.data if a.size else None, a.size, off.ctypes.data if m else None, ln.ctypes.data if m else None, m, out_align)
    st = lib().cz_seekable_locate_host(*args, 0, None, None, None, None, None, None, None, None, info.ctypes.data)
    k = 0 if st else int(info[0]["selected"])
    arr = [np.zeros(k, dtype=t) for t in (np.uint32, np.uint64, np.uint64, np.uint64, np.uint64, np.uint32, np.uint64)]
    spans = np.zeros(0 if st else m, dtype=SEEKABLE_SPAN_DTYPE)
    if not st:
        lib().cz_seekable_locate_host(*args, k, *[x.ctypes.data if k else None for x in arr], spans.ctypes.data if m else None, info.ctypes.data)
    return (info[0], *arr, spans)


def read_seekable(stream_or_index, ctx: Context, ranges, verify: bool = False, stream=None):
    """The bytes of `ranges`, a list of (offset, length) in the content of a seekable stream: a list of bytes, one per range.  Only
    the frames that hold a requested byte are decoded: the stream is staged in HBM, then index (unless a SeekableIndex is given, with
    the staged stream it was made from as the torch tensor `stream`), locate as a sizing call, locate, ONE decode_batch_device of the
    k frames, the gather and one copy back.  verify=True: the context verifies the frames' checksums, and where the table carries
    checksums they must equal the calculated ones.  Raises CzError on a malformed table, a range outside the content, a frame that
    fails (named by its number in the stream) or a checksum that differs."""
    import torch
    dev = torch.device(f"cuda:{ctx.device}")
    m = len(ranges)
    r = np.array(ranges, dtype=np.uint64).reshape(m, 2)
    if isinstance(stream_or_index, SeekableIndex):
        ix, own, d_stream = stream_or_index, False, stream
        if d_stream is None:
            raise CzError(status.CZ_E_INVALID_ARG, "read_seekable with a SeekableIndex needs the staged stream (stream=)")
    else:
        a = _as_u8(stream_or_index)
        d_stream = torch.zeros(a.size + 64, dtype=torch.uint8, device=dev)
        d_stream[:a.size] = torch.from_numpy(a.copy())
        torch.cuda.synchronize(dev)
        ix, own = ctx.seekable_index(d_stream.data_ptr(), a.size), True
    was = getattr(ctx, "_verify", False)
    try:
        d_rng = torch.from_numpy(np.ascontiguousarray(r.T).view(np.int64).copy()).to(dev) if m else torch.zeros((2, 1), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        rp = (d_rng[0].data_ptr(), d_rng[1].data_ptr(), m) if m else (0, 0, 0)
        size = ix.locate(*rp, 256)
        if int(size["status"]):
            raise CzError(int(size["status"]), f"cz_seekable_locate_device (range {int(size['detail'])})")
        k, dst_bytes = int(size["selected"]), int(size["dst_bytes"])
        if k == 0:
            return [b""] * m
        desc = torch.zeros((5, k), dtype=torch.int64, device=dev)       # in_off, in_len, out_off, out_cap, content_off
        d_u32 = torch.zeros((2, k), dtype=torch.int32, device=dev)      # frame, checksum
        d_spans = torch.zeros(m * SEEKABLE_SPAN_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_out = torch.zeros(int(size["out_bytes"]) + 256, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(k * RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_dst = torch.zeros(dst_bytes + 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        info = ix.locate(*rp, 256, k, d_u32[0].data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), desc[2].data_ptr(), desc[3].data_ptr(),
                         d_u32[1].data_ptr(), desc[4].data_ptr(), d_spans.data_ptr())
        if int(info["status"]):
            raise CzError(int(info["status"]), "cz_seekable_locate_device")
        if verify:
            ctx.set_verify_checksum(True)
        ctx.decode_batch_device(d_stream.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), k, d_out.data_ptr(), desc[2].data_ptr(),
                                desc[3].data_ptr(), d_res.data_ptr())
        ctx.seekable_gather_device(d_out.data_ptr(), desc[2].data_ptr(), desc[4].data_ptr(), k, rp[0], rp[1], d_spans.data_ptr(), m,
                                   d_dst.data_ptr(), dst_bytes)
        ctx.synchronize()
        res = d_res.cpu().numpy().view(RESULT_DTYPE)
        u32 = d_u32.cpu().numpy().view(np.uint32)
        for s in np.flatnonzero(res["status"] != 0)[:1]:
            raise CzError(int(res[s]["status"]), f"frame {int(u32[0][s])}")
        if verify and int(info["has_checksums"]):
            ok = ((res["flags"] & RESULT_CHECKSUM_COMPUTED) != 0) & (res["calculated_checksum"] == u32[1])
            for s in np.flatnonzero(~ok)[:1]:
                raise CzError(status.CZ_E_SEEK_TABLE, f"frame {int(u32[0][s])}: the table's checksum differs from the calculated one")
        out = d_dst.cpu().numpy()
        at = np.concatenate([[0], np.cumsum(r[:, 1])]).astype(np.uint64)
        return [out[int(at[j]): int(at[j + 1])].tobytes() for j in range(m)]
    finally:
        if verify:
            ctx.set_verify_checksum(was)
        if own:
            ix.close()


def _compress_flags(checksum, split, fse_tables, fast=False, records=False, fast_split=False, high=False, high_split=False) -> int:
    if high_split and (split or fse_tables or fast or records or fast_split or high):
        raise CzError(status.CZ_E_INVALID_ARG, "high_split goes with checksum alone: not with split, fse_tables, fast, records, fast_split or high")
    if high and (split or fse_tables or fast or records or fast_split):
        raise CzError(status.CZ_E_INVALID_ARG, "high goes with checksum alone: not with split, fse_tables, fast, records or fast_split")
    if fast_split and (split or fse_tables or fast or records):
        raise CzError(status.CZ_E_INVALID_ARG, "fast_split goes with checksum alone: not with split, fse_tables, fast or records")
    if records and (split or fse_tables or fast):
        raise CzError(status.CZ_E_INVALID_ARG, "records goes with checksum alone: not with split, fse_tables or fast")
    return ((COMPRESS_CHECKSUM if checksum else 0) | (COMPRESS_SPLIT if split else 0) | (COMPRESS_FSE_TABLES if fse_tables else 0)
            | (COMPRESS_FAST if fast else 0) | (COMPRESS_RECORDS if records else 0) | (COMPRESS_FAST_SPLIT if fast_split else 0)
            | (COMPRESS_HIGH if high else 0) | (COMPRESS_HIGH_SPLIT if high_split else 0))


def compress_bound(n: int) -> int:
    """cz_compress_bound: the largest frame cz_compress_batch_* writes for n input bytes."""
    return int(lib().cz_compress_bound(n))


def compress_split_segment() -> int:
    """cz_compress_split_segment: the segment size of COMPRESS_SPLIT in bytes."""
    return int(lib().cz_compress_split_segment())


def compress_record_max() -> int:
    """cz_compress_record_max: the largest input COMPRESS_RECORDS takes, in bytes."""
    return int(lib().cz_compress_record_max())


def compress_batch_host(buffers, ctx: Context, checksum: bool = False, split: bool = False, fse_tables: bool = False,
                        fast: bool = False, records: bool = False, fast_split: bool = False, high: bool = False,
                        high_split: bool = False):
    """Compresses every buffer into one zstd frame, in one launch: list of (result record, frame bytes).  split=True: buffers
    longer than compress_split_segment() are compressed by several workgroups side by side (COMPRESS_SPLIT).  fse_tables=True:
    the sequences of a block take FSE tables made for that block where they make it smaller (COMPRESS_FSE_TABLES).  fast=True:
    the fast level (COMPRESS_FAST), which the library refuses together with split or fse_tables.  records=True: the records level
    (COMPRESS_RECORDS) for buffers of at most compress_record_max() bytes, one wave each; not with the three before it.  fast_split=True: the fast
    level's frames, byte for byte, with the 128 KiB groups of one buffer on many workgroups (COMPRESS_FAST_SPLIT), for few, large
    buffers; with checksum alone.  high=True: the high-ratio level (COMPRESS_HIGH): the frame of fse_tables=True with sequences from
    two match tables, repeat-offset matches and a lazy parse; with checksum alone.  high_split=True: that level with the segments of
    one buffer (compress_split_segment() bytes each) on many workgroups (COMPRESS_HIGH_SPLIT), for few, large buffers; with checksum
    alone."""
    lens = np.array([len(b) for b in buffers], dtype=np.uint64)
    in_off = np.zeros(len(buffers), dtype=np.uint64)
    if len(buffers) > 1:
        in_off[1:] = np.cumsum(lens[:-1])
    in_base = np.frombuffer(b"".join(bytes(b) for b in buffers) + b"\0" * 16, dtype=np.uint8)
    caps = np.array([compress_bound(int(n)) for n in lens], dtype=np.uint64)
    out_off = np.zeros(len(buffers), dtype=np.uint64)
    if len(buffers) > 1:
        out_off[1:] = np.cumsum(caps[:-1])
    out = np.zeros(max(int(caps.sum()), 1), dtype=np.uint8)
    res = ctx.compress_batch_host(in_base, in_off, lens, out_off, caps, out, checksum=checksum, split=split, fse_tables=fse_tables,
                                  fast=fast, records=records, fast_split=fast_split, high=high, high_split=high_split)
    return [(res[i], out[int(out_off[i]): int(out_off[i]) + int(res[i]["bytes_written"])].tobytes()) for i in range(len(buffers))]


def compress_batch_host_dict(buffers, dict_index, ctx: Context, checksum: bool = False, dict_id: bool = True, records: bool = False,
                             fast_split: bool = False, high_split: bool = False):
    """As compress_batch_host, buffer i with dictionary dict_index[i] of ctx.set_compress_dictionaries (COMPRESS_NO_DICT: none;
    dict_index None: every buffer uses the one dictionary set): list of (result record, frame bytes).  records=True: the records
    level (COMPRESS_RECORDS).  fast_split=True (COMPRESS_FAST_SPLIT) and high_split=True (COMPRESS_HIGH_SPLIT) raise CzError: those levels
    take no dictionary."""
    lens = np.array([len(b) for b in buffers], dtype=np.uint64)
    in_off = np.zeros(len(buffers), dtype=np.uint64)
    if len(buffers) > 1:
        in_off[1:] = np.cumsum(lens[:-1])
    in_base = np.frombuffer(b"".join(bytes(b) for b in buffers) + b"\0" * 16, dtype=np.uint8)
    caps = np.array([compress_bound(int(n)) for n in lens], dtype=np.uint64)
    out_off = np.zeros(len(buffers), dtype=np.uint64)
    if len(buffers) > 1:
        out_off[1:] = np.cumsum(caps[:-1])
    out = np.zeros(max(int(caps.sum()), 1), dtype=np.uint8)
    res = ctx.compress_batch_dict_host(in_base, in_off, lens, out_off, caps, out, dict_index, checksum=checksum, dict_id=dict_id, records=records,
                                       fast_split=fast_split, high_split=high_split)
    return [(res[i], out[int(out_off[i]): int(out_off[i]) + int(res[i]["bytes_written"])].tobytes()) for i in range(len(buffers))]


def compress(data, ctx: Context, checksum: bool = False, split: bool = False, fse_tables: bool = False, fast: bool = False,
             records: bool = False, fast_split: bool = False, high: bool = False, high_split: bool = False) -> bytes:
    """One buffer -> one zstd frame (through the batched kernel; split=True: on many workgroups when it is large; fse_tables=True:
    per-block FSE tables for the sequences; fast=True: the fast level; records=True: the records level; fast_split=True: the fast
    level on many workgroups when the buffer is large; high=True: the high-ratio level; high_split=True: the high-ratio level on many
    workgroups when the buffer is large)."""
    (r, frame), = compress_batch_host([data], ctx, checksum=checksum, split=split, fse_tables=fse_tables, fast=fast, records=records,
                                      fast_split=fast_split, high=high, high_split=high_split)
    if int(r["status"]):
        raise CzError(int(r["status"]), "cz_compress_batch_host")
    return frame


def decode_batch_host(frames, caps, ctx: Context | None = None):
    """Convenience: list of frame byte strings -> list of (result record, decoded bytes)."""
    own = ctx is None
    ctx = ctx or Context()
    try:
        lens = np.array([len(f) for f in frames], dtype=np.uint64)
        in_off = np.zeros(len(frames), dtype=np.uint64)
        if len(frames) > 1:
            in_off[1:] = np.cumsum(lens[:-1])
        in_base = np.frombuffer(b"".join(frames) + b"\0" * 16, dtype=np.uint8)
        caps = np.array(caps, dtype=np.uint64)
        pad = (caps + np.uint64(255)) // np.uint64(256) * np.uint64(256)
        out_off = np.zeros(len(frames), dtype=np.uint64)
        if len(frames) > 1:
            out_off[1:] = np.cumsum(pad[:-1])
        total = int(pad.sum())
        out, res = ctx.decode_batch_host(in_base, in_off, lens, out_off, caps, total)
        return [(res[i], out[int(out_off[i]): int(out_off[i]) + min(int(res[i]["bytes_produced"]), int(caps[i]))].tobytes())
                for i in range(len(frames))]
    finally:
        if own:
            ctx.close()


def partition_balanced(weights, parts: int) -> np.ndarray:
    """cz_partition_balanced: deals items to `parts` parts by weight (heaviest first, to the lightest part).  No device needed."""
    w = np.ascontiguousarray(weights, dtype=np.uint64)
    out = np.zeros(w.size, dtype=np.uint32)
    st = lib().cz_partition_balanced(w.ctypes.data if w.size else None, w.size, parts, out.ctypes.data if w.size else None)
    if st:
        raise CzError(st, "cz_partition_balanced")
    return out


def decode_batch_multi(frames, caps, ctxs):
    """cz_decode_batch_multi: one batch over several contexts (one per GPU).  Returns ([(result, bytes)], device_of)."""
    lens = np.array([len(f) for f in frames], dtype=np.uint64)
    in_off = np.zeros(len(frames), dtype=np.uint64)
    if len(frames) > 1:
        in_off[1:] = np.cumsum(lens[:-1])
    in_base = np.frombuffer(b"".join(frames) + b"\0" * 16, dtype=np.uint8)
    caps = np.array(caps, dtype=np.uint64)
    pad = (caps + np.uint64(255)) // np.uint64(256) * np.uint64(256)
    out_off = np.zeros(len(frames), dtype=np.uint64)
    if len(frames) > 1:
        out_off[1:] = np.cumsum(pad[:-1])
    total = int(pad.sum())
    out = np.zeros(total + 16, dtype=np.uint8)
    res = np.zeros(len(frames), dtype=RESULT_DTYPE)
    dev = np.zeros(len(frames), dtype=np.uint32)
    handles = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    st = lib().cz_decode_batch_multi(handles, len(ctxs), in_base.ctypes.data, in_base.size, in_off.ctypes.data, lens.ctypes.data, len(frames),
                                     out.ctypes.data, total, out_off.ctypes.data, caps.ctypes.data, res.ctypes.data, dev.ctypes.data)
    if st:
        raise CzError(st, "cz_decode_batch_multi")
    return [(res[i], out[int(out_off[i]): int(out_off[i]) + min(int(res[i]["bytes_produced"]), int(caps[i]))].tobytes()) for i in range(len(frames))], dev


def decode_batch_multi_device(ctxs, shares):
    """cz_decode_batch_multi_device: shares = per context (d_in_base, d_in_off, d_in_len, n, d_out_base, d_out_off, d_out_cap, d_results),
    all device pointers of that context's device.  Only enqueues."""
    from ._lib import DeviceShare
    arr = (DeviceShare * len(ctxs))(*[DeviceShare(*[int(v) for v in sh]) for sh in shares])
    handles = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    st = lib().cz_decode_batch_multi_device(handles, len(ctxs), arr)
    if st:
        raise CzError(st, "cz_decode_batch_multi_device")


def gather_to_root(ctxs, root, d_src, nbytes, d_dst_on_root):
    """cz_gather_to_root: concurrent peer copies of the other contexts' decoded arenas to the root context's device."""
    k = len(ctxs)
    handles = (C.c_void_p * k)(*[c._h for c in ctxs])
    src = (C.c_void_p * k)(*[int(v) for v in d_src])
    dst = (C.c_void_p * k)(*[int(v) for v in d_dst_on_root])
    nb = (C.c_size_t * k)(*[int(v) for v in nbytes])
    st = lib().cz_gather_to_root(handles, k, int(root), src, nb, dst)
    if st:
        raise CzError(st, "cz_gather_to_root")


def read_frame_header(src):
    """read_frame_header (src/frame.cairo:152-284).  Returns (status, FrameHeader, detail)."""
    a = _as_u8(src)
    fh = FrameHeader()
    detail = (C.c_uint64 * 2)()
    st = lib().cz_read_frame_header(a.ctypes.data if a.size else None, a.size, C.byref(fh), detail)
    return st, fh, (detail[0], detail[1])


def read_block_header(src):
    """BlockDecoderTrait::read_block_header (src/decoding/block_decoder.cairo:237-278)."""
    a = _as_u8(src)
    bh = BlockHeader()
    st = lib().cz_read_block_header(a.ctypes.data if a.size else None, a.size, C.byref(bh))
    return st, bh


STREAM_ENTRY_DTYPE = np.dtype([("offset", "<u8"), ("length", "<u8"), ("kind", "<u4"), ("magic", "<u4"), ("content_size", "<u8"),
                               ("out_bound", "<u8"), ("window_size", "<u8")])
STREAM_FRAME, STREAM_SKIPPABLE = 0, 1


def stream_split(src):
    """cz_stream_split: cuts a stream of concatenated zstd / skippable frames (the caller's side of SkipFrame,
    src/frame.cairo:160-166) into entries.  Returns (status, entries, consumed)."""
    a = _as_u8(src)
    cap = 64
    while True:
        ents = np.zeros(cap, dtype=STREAM_ENTRY_DTYPE)
        count, consumed = C.c_size_t(), C.c_size_t()
        st = lib().cz_stream_split(a.ctypes.data if a.size else None, a.size, ents.ctypes.data, cap, C.byref(count), C.byref(consumed))
        if st == status.CZ_E_TARGET_TOO_SMALL:
            cap = count.value
            continue
        return st, ents[: min(count.value, cap)], consumed.value


def decode_stream(src, ctx: "Context | None" = None) -> bytes:
    """Decodes every zstd frame of a multi-frame stream in ONE batch launch (skippable frames are skipped) and
    returns the concatenated output.  Raises CzError on a malformed stream or frame."""
    a = _as_u8(src)
    st, ents, consumed = stream_split(a)
    if st:
        raise CzError(st, f"cz_stream_split stopped at byte {consumed}")
    fr = ents[ents["kind"] == STREAM_FRAME]
    frames = [a[int(e["offset"]): int(e["offset"] + e["length"])] for e in fr]
    caps = [int(e["out_bound"]) + 64 for e in fr]
    out = []
    for (r, o), e in zip(decode_batch_host(frames, caps, ctx), fr):
        if int(r["status"]):
            raise CzError(int(r["status"]), f"frame at byte {int(e['offset'])}")
        out.append(o)
    return b"".join(out)


class DecoderScratch:
    """DecoderScratch (src/decoding/scratch.cairo:11-67) resident on the device."""

    def __init__(self, ctx: "Context", window_size: int = 0, _borrowed=None):
        self._ctx, self._own = ctx, _borrowed is None
        if _borrowed is not None:
            self._h = _borrowed
            return
        self._h = C.c_void_p()
        st = lib().cz_decoder_scratch_create(ctx._h, window_size, C.byref(self._h))
        if st:
            self._h = None
            raise CzError(st, "cz_decoder_scratch_create")
        ctx._decoders.add(self)

    def close(self):
        if getattr(self, "_h", None) and self._own:
            lib().cz_decoder_scratch_destroy(self._h)
        self._h = None

    __del__ = close

    def reset(self, window_size: int):
        return lib().cz_decoder_scratch_reset(self._h, window_size)

    def buffer_len(self) -> int:
        return int(lib().cz_decoder_scratch_buffer_len(self._h))

    def total_output(self) -> int:
        return int(lib().cz_decoder_scratch_total_output(self._h))

    def drain(self, cap: int = 1 << 24) -> bytes:
        out = np.empty(max(cap, 1), dtype=np.uint8)
        w = C.c_size_t()
        st = lib().cz_decoder_scratch_drain(self._h, out.ctypes.data, cap, C.byref(w))
        if st:
            raise CzError(st, "cz_decoder_scratch_drain")
        return out[: w.value].tobytes()

    def drain_to_window_size(self, cap: int = 1 << 24):
        out = np.empty(max(cap, 1), dtype=np.uint8)
        w = C.c_size_t()
        rc = lib().cz_decoder_scratch_drain_to_window_size(self._h, out.ctypes.data, cap, C.byref(w))
        if rc < 0:
            raise CzError(-rc, "cz_decoder_scratch_drain_to_window_size")
        return out[: w.value].tobytes() if rc == 1 else None

    def hash_digest(self) -> int:
        return int(lib().cz_decoder_scratch_hash_digest(self._h))

    def init_from_dict(self, dictionary: "Dictionary") -> int:
        """DecoderScratchTrait::init_from_dict (src/decoding/scratch.cairo:60-65)."""
        self._dict = dictionary                                        # keep it alive while the workspace uses it
        return lib().cz_decoder_scratch_init_from_dict(self._h, dictionary._h)


class Dictionary:
    """Dictionary / DictionaryTrait::decode_dict (src/decoding/dictionary.cairo:11-91), parsed on and resident in the device."""

    def __init__(self, ctx: "Context", raw):
        a = _as_u8(raw)
        self._ctx, self._h = ctx, C.c_void_p()
        detail = (C.c_uint64 * 2)()
        st = lib().cz_dictionary_decode(ctx._h, a.ctypes.data if a.size else None, a.size, C.byref(self._h), detail)
        if st:
            self._h = None
            raise CzError(st, f"cz_dictionary_decode (detail {int(detail[0]):#x})")
        ctx._decoders.add(self)

    def close(self):
        if getattr(self, "_h", None):
            lib().cz_dictionary_destroy(self._h)
        self._h = None

    __del__ = close

    @property
    def id(self) -> int:
        return int(lib().cz_dictionary_id(self._h))

    @property
    def content_len(self) -> int:
        return int(lib().cz_dictionary_content_len(self._h))

    @property
    def offset_hist(self):
        v = (C.c_uint32 * 3)()
        lib().cz_dictionary_offset_hist(self._h, v)
        return tuple(int(x) for x in v)


def decode_frame_with_dict(src, dictionary: Dictionary, ctx: "Context") -> bytes:
    """One frame, block by block, on a workspace seeded from `dictionary`: read_frame_header -> DecoderScratch::new ->
    init_from_dict -> {read_block_header, decode_block_content} until the last block -> drain.  (The reference's
    FrameDecoder never calls init_from_dict, so neither does cz_frame_decoder_*.)  Raises CzError."""
    a = _as_u8(src)
    st, fh, _ = read_frame_header(a)
    if st:
        raise CzError(st, "read_frame_header")
    ws = DecoderScratch(ctx, int(fh.window_size))
    try:
        st = ws.init_from_dict(dictionary)
        if st:
            raise CzError(st, "init_from_dict")
        bd, pos = BlockDecoder(), int(fh.header_len)
        while True:
            st, bh, used = bd.read_block_header(a[pos:])
            if st:
                raise CzError(st, f"read_block_header at byte {pos}")
            pos += used
            st, used = bd.decode_block_content(bh, ws, a[pos:])
            if st:
                raise CzError(st, f"decode_block_content at byte {pos}")
            pos += used
            if bh.last_block:
                return ws.drain(max(ws.buffer_len(), 1))
    finally:
        ws.close()


class BlockDecoder:
    """BlockDecoder (src/decoding/block_decoder.cairo:20-30, :69-137, :237-278)."""

    class _State(C.Structure):
        _fields_ = [("internal_state", C.c_uint8), ("header_buffer", C.c_uint8 * 3)]

    READY_FOR_HEADER, READY_FOR_BODY, FAILED = 0, 1, 2

    def __init__(self):
        self._s = BlockDecoder._State()
        lib().cz_block_decoder_new(C.byref(self._s))

    @property
    def internal_state(self) -> int:
        return int(self._s.internal_state)

    def read_block_header(self, src):
        """Returns (status, BlockHeader, consumed)."""
        a = _as_u8(src)
        bh = BlockHeader()
        used = C.c_uint8()
        st = lib().cz_block_decoder_read_block_header(C.byref(self._s), a.ctypes.data if a.size else None, a.size, C.byref(bh), C.byref(used))
        return st, bh, int(used.value)

    def decode_block_content(self, header, workspace: DecoderScratch, src):
        """Returns (status, bytes of src the block took)."""
        a = _as_u8(src)
        used = C.c_uint64()
        st = lib().cz_block_decoder_decode_block_content(C.byref(self._s), C.byref(header), workspace._h, a.ctypes.data if a.size else None, a.size, C.byref(used))
        return st, int(used.value)


class BlockDecodingStrategy:
    """src/frame_decoder.cairo:33-37"""
    ALL, UPTO_BLOCKS, UPTO_BYTES = 0, 1, 2


class FrameDecoder:
    """Mirror of FrameDecoder / FrameDecoderTrait (src/frame_decoder.cairo:17-335).  Methods
    return the status code where the reference returns Result<_, FrameDecoderError>."""

    def __init__(self, ctx: Context):
        self._ctx = ctx
        self._h = C.c_void_p()
        st = lib().cz_frame_decoder_create(ctx._h, C.byref(self._h))
        if st:
            self._h = None
            raise CzError(st, "cz_frame_decoder_create")
        ctx._decoders.add(self)

    def close(self):
        if getattr(self, "_h", None):
            lib().cz_frame_decoder_destroy(self._h)
            self._h = None

    __del__ = close

    def scratch(self) -> "DecoderScratch":
        """FrameDecoderState.decoder_scratch (src/frame_decoder.cairo:25), owned by this frame decoder."""
        return DecoderScratch(self._ctx, _borrowed=C.c_void_p(lib().cz_frame_decoder_scratch(self._h)))

    def _init(self, fn, src):
        a = _as_u8(src)
        consumed = C.c_size_t()
        detail = (C.c_uint64 * 2)()
        st = fn(self._h, a.ctypes.data if a.size else None, a.size, C.byref(consumed), detail)
        return st, consumed.value, (detail[0], detail[1])

    def new(self, src):
        return self._init(lib().cz_frame_decoder_new, src)

    def reset(self, src):
        return self._init(lib().cz_frame_decoder_reset, src)

    def content_size(self):
        return lib().cz_frame_decoder_content_size(self._h)

    def get_checksum_from_data(self):
        v = C.c_uint32()
        return v.value if lib().cz_frame_decoder_checksum_from_data(self._h, C.byref(v)) else None

    def get_calculated_checksum(self):
        return lib().cz_frame_decoder_calculated_checksum(self._h)

    def bytes_read_from_source(self):
        return lib().cz_frame_decoder_bytes_read_from_source(self._h)

    def is_finished(self):
        return bool(lib().cz_frame_decoder_is_finished(self._h))

    def blocks_decoded(self):
        return lib().cz_frame_decoder_blocks_decoded(self._h)

    def decode_blocks(self, src, strategy=BlockDecodingStrategy.ALL, n=0):
        a = _as_u8(src)
        consumed = C.c_size_t()
        fin = C.c_int()
        st = lib().cz_frame_decoder_decode_blocks(self._h, a.ctypes.data if a.size else None, a.size, strategy, n,
                                                  C.byref(consumed), C.byref(fin))
        return st, consumed.value, bool(fin.value)

    def can_collect(self):
        return lib().cz_frame_decoder_can_collect(self._h)

    def collect(self, cap: int = 1 << 24):
        out = np.empty(cap, dtype=np.uint8)
        w = C.c_size_t()
        r = lib().cz_frame_decoder_collect(self._h, out.ctypes.data, cap, C.byref(w))
        if r < 0:
            raise CzError(-r, "collect")
        return out[: w.value].tobytes() if r == 1 else None

    def read(self, cap: int = 1 << 24):
        out = np.empty(cap, dtype=np.uint8)
        n = lib().cz_frame_decoder_read(self._h, out.ctypes.data, cap)
        return out[:n].tobytes()

    def decode_from_to(self, src, cap: int = 1 << 24):
        a = _as_u8(src)
        out = np.empty(cap, dtype=np.uint8)
        r, w = C.c_size_t(), C.c_size_t()
        st = lib().cz_frame_decoder_decode_from_to(self._h, a.ctypes.data if a.size else None, a.size, out.ctypes.data, cap,
                                                   C.byref(r), C.byref(w))
        return st, r.value, out[: w.value].tobytes()
