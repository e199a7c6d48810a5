"""Runs the fast compression level (CZ_COMPRESS_FAST, cz_compress_frames_fast_kernel) on the CPU SIMT emulator:
tests/emu/emu_encode_fast.cpp, built by tests/emu/Makefile under ASan/UBSan.  Test infrastructure only."""
import struct

import emu_common
from emu_common import EMU_DIR, COMPRESS_RESULT_DTYPE, compress_bound  # noqa: F401  (re-exported)

CHECKSUM, FAST = 1, 32
SUB, GROUP = 32 << 10, 128 << 10       # the kernel's sub-block and group (checked against what the binary reports)


def build():
    return emu_common.build("emu_encode_fast")


def run(buffers, caps=None, flags=FAST, timeout=900):
    """[(result record, whole output region — 0xEE where nothing was written)] per buffer."""
    caps = emu_common.compress_caps(buffers, caps)
    (raw,), _ = emu_common.execute("emu_encode_fast", emu_common.compress_batch(buffers, caps, flags), timeout)
    assert struct.unpack_from("<QQ", raw, 0) == (SUB, GROUP)
    return emu_common.results(raw, 16, COMPRESS_RESULT_DTYPE, caps)
