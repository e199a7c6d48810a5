"""Runs the batched compressor (cz_compress_frames_kernel) on the CPU SIMT emulator: tests/emu/emu_encode.cpp, built by
tests/emu/Makefile under ASan/UBSan.  Test infrastructure only."""
import emu_common
from emu_common import EMU_DIR, COMPRESS_RESULT_DTYPE, compress_bound  # noqa: F401  (re-exported)

CHECKSUM = 1


def build():
    return emu_common.build("emu_encode")


def run(buffers, caps=None, flags=0, timeout=900):
    """[(result record, whole output region — 0xEE where nothing was written)] per buffer."""
    caps = emu_common.compress_caps(buffers, caps)
    (raw,), _ = emu_common.execute("emu_encode", emu_common.compress_batch(buffers, caps, flags), timeout)
    return emu_common.results(raw, 0, COMPRESS_RESULT_DTYPE, caps)
