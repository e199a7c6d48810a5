"""Runs CZ_COMPRESS_HIGH (cz_compress_frames_high_kernel) and, for the comparisons, CZ_COMPRESS_FSE_TABLES
(cz_compress_frames_fse_kernel) on the CPU SIMT emulator: tests/emu/emu_encode_high.cpp, built under ASan/UBSan by
tests/emu/high.mk, which takes its flags and dependencies from tests/emu/Makefile.  Test infrastructure only."""
import fcntl
import os
import subprocess
import tempfile

import emu_common
from emu_common import EMU_DIR, COMPRESS_RESULT_DTYPE, compress_bound  # noqa: F401  (re-exported)

CHECKSUM, FSE_TABLES, HIGH = 1, 16, 256
TARGET = "emu_encode_high"


def build():
    with open(os.path.join(EMU_DIR, f".{TARGET}.lock"), "w") as lk:         # several test workers may ask at once
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", EMU_DIR, "-f", "high.mk", TARGET], stdout=subprocess.DEVNULL)
    return os.path.join(EMU_DIR, TARGET)


def run(buffers, caps=None, flags=HIGH, timeout=900):
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
    return emu_common.results(raw, 0, COMPRESS_RESULT_DTYPE, caps)
