"""Runs the seekable-read cases of tests/emu/seekable_read_cases.h on either of two programs built by tests/emu/seekable_read.mk
under ASan/UBSan: `seekable_read_host_main` (csrc/czstd_seekable_read_host.h alone, g++) and `emu_seekable_read` (the kernels of
czstd_seekable_read.hip on the CPU SIMT emulator).  Test infrastructure only."""
import fcntl
import os
import struct
import subprocess
import tempfile

import numpy as np

from emu_common import EMU_DIR
from seekable_runner import INFO_DTYPE

HOST, EMU = "seekable_read_host_main", "emu_seekable_read"
READ_INFO_DTYPE = np.dtype([("status", "<i4"), ("reason", "<u4"), ("frames", "<u8"), ("content_bytes", "<u8"), ("selected", "<u8"),
                            ("out_bytes", "<u8"), ("dst_bytes", "<u8"), ("detail", "<u8"), ("has_checksums", "<u4"), ("reserved", "<u4")])
SPAN_DTYPE = np.dtype([("dst_off", "<u8"), ("src_off", "<u8"), ("sel_first", "<u4"), ("sel_count", "<u4")])
ARRAY_TYPES = ("<u4", "<u8", "<u8", "<u8", "<u8", "<u4", "<u8")           # frame, in_off, in_len, out_off, out_cap, checksum, content_off
assert READ_INFO_DTYPE.itemsize == 64 and SPAN_DTYPE.itemsize == 24


def build(target):
    with open(os.path.join(EMU_DIR, f".{target if target.startswith('emu_') else 'emu_' + target}.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", EMU_DIR, "-f", "seekable_read.mk", target], stdout=subprocess.DEVNULL)
    return os.path.join(EMU_DIR, target)


def call(ranges, align=1, frames_cap=0, k=0, arrays=True):
    """One locate of an 'L' case: `ranges` a list of (offset, length); k: the entries of every per-frame array block."""
    m = len(ranges)
    r = np.array(ranges, dtype=np.uint64).reshape(m, 2)
    return b"".join([struct.pack("<Q", m), r[:, 0].tobytes(), r[:, 1].tobytes(), struct.pack("<IQQB", align, frames_cap, k, int(arrays))])


def locate_case(stream, calls):
    return b"".join([b"L", struct.pack("<Q", len(stream)), bytes(stream), struct.pack("<I", len(calls))] + list(calls))


def spans_array(spans):
    a = np.zeros(len(spans), dtype=SPAN_DTYPE)
    for j, sp in enumerate(spans):
        a[j] = sp
    return a


def gather_case(out_off, content_off, decoded, ranges, spans, dst_bytes, residue=0):
    """One 'G' case: the arrays of a locate (from the model), the decoded buffer, the ranges and their spans (a SPAN_DTYPE array)."""
    m = len(ranges)
    r = np.array(ranges, dtype=np.uint64).reshape(m, 2)
    return b"".join([b"G", struct.pack("<IQ", residue, len(out_off)), np.array(out_off, dtype=np.uint64).tobytes(),
                     np.array(content_off, dtype=np.uint64).tobytes(), struct.pack("<Q", len(decoded)), bytes(decoded), struct.pack("<Q", m),
                     r[:, 0].tobytes(), r[:, 1].tobytes(), spans.tobytes(), struct.pack("<Q", dst_bytes)])


def run(target, cases, timeout=900):
    """The results of `cases` (a list of locate_case / gather_case bytes), in order: for an 'L' case (ret, info of the table, [per
    call (ret, read info, clean, [the seven arrays], spans)]), for a 'G' case (ret, block bytes); and with target EMU the gather's
    tile in bytes up front."""
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
        if c[:1] == b"G":
            n = struct.unpack_from("<Q", raw, pos + 4)[0]
            out.append((ret, raw[pos + 12:pos + 12 + n]))
            pos += 12 + n
            continue
        table = np.frombuffer(raw, dtype=INFO_DTYPE, count=1, offset=pos + 4)[0]
        pos += 60
        ln = struct.unpack_from("<Q", c, 1)[0]
        ncalls = struct.unpack_from("<I", c, 9 + ln)[0] if ret == 0 else 0
        calls = []
        for _ in range(ncalls):
            cret = struct.unpack_from("<i", raw, pos)[0]
            info = np.frombuffer(raw, dtype=READ_INFO_DTYPE, count=1, offset=pos + 4)[0]
            clean, k = struct.unpack_from("<BQ", raw, pos + 68)
            pos += 77
            arrays = []
            for t in ARRAY_TYPES:
                arrays.append(np.frombuffer(raw, dtype=t, count=k, offset=pos))
                pos += k * np.dtype(t).itemsize
            m = struct.unpack_from("<Q", raw, pos)[0]
            spans = np.frombuffer(raw, dtype=SPAN_DTYPE, count=m, offset=pos + 8)
            pos += 8 + 24 * m
            calls.append((cret, info, clean, arrays, spans))
        out.append((ret, table, calls))
    assert pos == len(raw)
    return out
