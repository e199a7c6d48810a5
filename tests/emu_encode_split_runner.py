"""Runs the split compressor (CZ_COMPRESS_SPLIT: cz_compress_plan_kernel, cz_compress_segments_kernel) on the CPU SIMT emulator:
tests/emu/emu_encode_split.cpp, built by tests/emu/Makefile under ASan/UBSan with one-block segments and a small
overlap.  Test infrastructure only."""
import struct

import emu_common
from emu_common import EMU_DIR, COMPRESS_RESULT_DTYPE, compress_bound  # noqa: F401  (re-exported)

CHECKSUM, SPLIT = 1, 4
S, W = 128 << 10, 8 << 10              # the emulator build's segment and overlap (checked against what the binary reports)


def build():
    return emu_common.build("emu_encode_split")


def run(buffers, caps=None, flags=SPLIT, timeout=900):
    """[(result record, whole output region — 0xEE where nothing was written)] per buffer."""
    caps = emu_common.compress_caps(buffers, caps)
    (raw,), _ = emu_common.execute("emu_encode_split", emu_common.compress_batch(buffers, caps, flags), timeout)
    assert struct.unpack_from("<QQ", raw, 0) == (S, W)
    return emu_common.results(raw, 16, COMPRESS_RESULT_DTYPE, caps)
