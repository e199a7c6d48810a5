"""Runs CZ_COMPRESS_HIGH_SPLIT (cz_compress_plan_kernel, cz_compress_segments_high_kernel) and, for the comparisons, CZ_COMPRESS_HIGH
(cz_compress_frames_high_kernel) and CZ_COMPRESS_SPLIT | CZ_COMPRESS_FSE_TABLES (cz_compress_segments_fse_kernel) on the CPU SIMT
emulator: tests/emu/emu_encode_high_split.cpp, built under ASan/UBSan by tests/emu/high_split.mk with one-block segments and an
8 KiB overlap; the flags and dependencies are those of tests/emu/Makefile.  Test infrastructure only."""
import fcntl
import os
import struct
import subprocess
import tempfile

import emu_common
from emu_common import EMU_DIR, COMPRESS_RESULT_DTYPE, compress_bound  # noqa: F401  (re-exported)

CHECKSUM, SPLIT, FSE_TABLES, HIGH, HIGH_SPLIT = 1, 4, 16, 256, 512
S, W = 128 << 10, 8 << 10              # the emulator build's segment and overlap (checked against what the binary reports)
TARGET = "emu_encode_high_split"


def build():
    with open(os.path.join(EMU_DIR, f".{TARGET}.lock"), "w") as lk:         # several test workers may ask at once
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", EMU_DIR, "-f", "high_split.mk", TARGET], stdout=subprocess.DEVNULL)
    return os.path.join(EMU_DIR, TARGET)


def run(buffers, caps=None, flags=HIGH_SPLIT, timeout=900):
    """[(result record, whole output region — 0xEE where nothing was written)] per buffer."""
    caps = emu_common.compress_caps(buffers, caps)
    exe = build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(emu_common.compress_batch(buffers, caps, flags))
        p = subprocess.run([exe, inp, outp], capture_output=True, timeout=timeout, env=env)
        if p.returncode != 0:
            raise RuntimeError(f"{TARGET} failed rc={p.returncode}\n{p.stderr.decode()[-4000:]}")
        with open(outp, "rb") as f:
            raw = f.read()
    assert struct.unpack_from("<QQ", raw, 0) == (S, W)
    return emu_common.results(raw, 16, COMPRESS_RESULT_DTYPE, caps)
