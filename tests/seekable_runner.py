"""Runs the seekable-stream cases of tests/emu/seekable_cases.h on either of two programs built by tests/emu/seekable.mk under
ASan/UBSan: `seekable_host_main` (csrc/czstd_seekable_host.h alone, g++) and `emu_seekable` (the kernels of czstd_seekable.hip on the
CPU SIMT emulator).  Also the frames and records the seekable tests share.  Test infrastructure only."""
import ctypes
import fcntl
import os
import struct
import subprocess
import tempfile

import numpy as np

from emu_common import COMPRESS_RESULT_DTYPE, EMU_DIR

HOST, EMU = "seekable_host_main", "emu_seekable"
INFO_DTYPE = np.dtype([("status", "<i4"), ("reason", "<u4"), ("frames", "<u8"), ("frames_bytes", "<u8"), ("content_bytes", "<u8"),
                       ("stream_bytes", "<u8"), ("detail", "<u8"), ("has_checksums", "<u4"), ("reserved", "<u4")])
CHECKSUMS = 1
ALL = 0xFFFFFFFFFFFFFFFF


def build(target):
    with open(os.path.join(EMU_DIR, f".{target if target.startswith('emu_') else 'emu_' + target}.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", EMU_DIR, "-f", "seekable.mk", target], stdout=subprocess.DEVNULL)
    return os.path.join(EMU_DIR, target)


def records(lengths, sizes, checksums=None):
    """cz_compress_result records of frames that went well."""
    r = np.zeros(len(lengths), dtype=COMPRESS_RESULT_DTYPE)
    r["bytes_written"], r["bytes_read"], r["blocks"] = lengths, sizes, 1
    if checksums is not None:
        r["checksum"], r["flags"] = checksums, 1
    return r


def pack_case(frames, recs, flags=0, cap=None, residue=0):
    """One 'P' case: `frames` are the bytes in each slot (what the record says need not agree with them)."""
    if cap is None:
        cap = sum(len(f) for f in frames) + 17 + len(frames) * (12 if flags & 1 else 8)
    out = [b"P", struct.pack("<IIQQ", flags, residue, cap, len(frames))]
    for f, r in zip(frames, recs):
        out += [r.tobytes(), struct.pack("<Q", len(f)), bytes(f)]
    return b"".join(out)


def open_case(stream, first=0, count=ALL, align=1, k=0, arrays=True, residue=1):
    return b"".join([b"O", struct.pack("<IQ", residue, len(stream)), bytes(stream), struct.pack("<QQIQB", first, count, align, k, int(arrays))])


def run(target, cases, timeout=900):
    """The results of `cases` (a list of pack_case / open_case bytes), in order: for a pack (ret, info, block bytes), for an open
    (ret, info, in_off, in_len, out_off, out_cap, checksums); and with target EMU the gather's tile in bytes up front."""
    exe = build(target)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(b"".join(cases))
        p = subprocess.run([exe, inp, outp], capture_output=True, timeout=timeout, env=env)
        if p.returncode != 0:
            raise RuntimeError(f"{target} failed rc={p.returncode}\n{p.stderr.decode()[-4000:]}")
        raw = open(outp, "rb").read()
    pos, out = 0, []
    if target == EMU:
        out.append(struct.unpack_from("<Q", raw, 0)[0])
        pos = 8
    for c in cases:
        ret = struct.unpack_from("<i", raw, pos)[0]
        info = np.frombuffer(raw, dtype=INFO_DTYPE, count=1, offset=pos + 4)[0]
        n = struct.unpack_from("<Q", raw, pos + 60)[0]
        pos += 68
        if c[:1] == b"P":
            out.append((ret, info, raw[pos:pos + n]))
            pos += n
        else:
            arr = [np.frombuffer(raw, dtype="<u8", count=n, offset=pos + 8 * n * j) for j in range(4)]
            arr.append(np.frombuffer(raw, dtype="<u4", count=n, offset=pos + 32 * n))
            out.append((ret, info, *arr))
            pos += 36 * n
    assert pos == len(raw)
    return out


_zstd = None


def zstd_frame(data, checksum=False):
    """One libzstd frame of `data` (level 1)."""
    global _zstd
    if _zstd is None:
        z = ctypes.CDLL("libzstd.so.1")
        z.ZSTD_compressBound.restype = ctypes.c_size_t
        z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
        z.ZSTD_createCCtx.restype = ctypes.c_void_p
        z.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        z.ZSTD_compress2.restype = ctypes.c_size_t
        z.ZSTD_compress2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        z.ZSTD_isError.restype = ctypes.c_uint
        z.ZSTD_isError.argtypes = [ctypes.c_size_t]
        z.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
        _zstd = z
    z = _zstd
    cctx = z.ZSTD_createCCtx()
    z.ZSTD_CCtx_setParameter(cctx, 100, 1)                              # ZSTD_c_compressionLevel
    z.ZSTD_CCtx_setParameter(cctx, 201, int(checksum))                  # ZSTD_c_checksumFlag
    cap = z.ZSTD_compressBound(len(data))
    dst = ctypes.create_string_buffer(cap)
    src = ctypes.create_string_buffer(bytes(data), max(len(data), 1))
    n = z.ZSTD_compress2(cctx, dst, cap, src, len(data))
    z.ZSTD_freeCCtx(cctx)
    assert not z.ZSTD_isError(n)
    return dst.raw[:n]


def contents(n, big=()):
    """n contents of lengths 0..40 in a cycle, those at the indices in `big` of 200 KiB: text-like, each different."""
    rng = np.random.default_rng(77)
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(200)]
    pool = b" ".join(words[int(i)] for i in rng.integers(0, 200, 60000))
    return [pool[3 * i: 3 * i + ((200 << 10) if i in big else i % 41)] for i in range(n)]
