"""Runs the fast compression level (CZ_COMPRESS_FAST, cz_compress_frames_fast_kernel) on the CPU SIMT emulator:
tests/emu/emu_encode_fast.cpp, built by tests/emu/Makefile.encode_fast under ASan/UBSan.  Test infrastructure only."""
import fcntl
import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
COMPRESS_RESULT_DTYPE = np.dtype([("status", "<i4"), ("blocks", "<u4"), ("bytes_read", "<u8"), ("bytes_written", "<u8"),
                                  ("checksum", "<u4"), ("flags", "<u4")])
CHECKSUM, FAST = 1, 32
SUB, GROUP = 32 << 10, 128 << 10       # the kernel's sub-block and group (checked against what the binary reports)


def build():
    with open(os.path.join(EMU_DIR, ".emu_encode_fast.lock"), "w") as lk:          # several test workers may ask at once
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", EMU_DIR, "-f", "Makefile.encode_fast", "emu_encode_fast"], stdout=subprocess.DEVNULL)
    return os.path.join(EMU_DIR, "emu_encode_fast")


def compress_bound(n: int) -> int:
    """cz_compress_bound, restated (the emulator has no host library)."""
    blocks = (n + (128 << 10) - 1) // (128 << 10) if n else 1
    return 18 + 3 * blocks + n


def run(buffers, caps=None, flags=FAST, timeout=900):
    """[(result record, whole output region — 0xEE where nothing was written)] per buffer."""
    exe = build()
    caps = [compress_bound(len(b)) for b in buffers] if caps is None else list(caps)
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<QI", len(buffers), flags))
            for b, cap in zip(buffers, caps):
                f.write(struct.pack("<QQ", len(b), cap))
                f.write(bytes(b))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        p = subprocess.run([exe, inp, outp], capture_output=True, timeout=timeout, env=env)
        if p.returncode != 0:
            raise RuntimeError(f"emu_encode_fast failed rc={p.returncode}\n{p.stderr.decode()[-4000:]}")
        raw = open(outp, "rb").read()
    assert struct.unpack_from("<QQ", raw, 0) == (SUB, GROUP)
    out, pos = [], 16
    for cap in caps:
        r = np.frombuffer(raw, dtype=COMPRESS_RESULT_DTYPE, count=1, offset=pos)[0]
        pos += COMPRESS_RESULT_DTYPE.itemsize
        out.append((r, raw[pos:pos + cap]))
        pos += cap
    return out
