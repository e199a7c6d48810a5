"""Runs the compressor with and without CZ_COMPRESS_FSE_TABLES on the CPU SIMT emulator: tests/emu/emu_encode_fse.cpp, built by
tests/emu/Makefile under ASan/UBSan with one-block segments and a small overlap.  The flags pick the kernel as the host
library does (frames / segments, each plain or with per-block FSE tables).  Test infrastructure only."""
import struct

import emu_common
from emu_common import EMU_DIR, COMPRESS_RESULT_DTYPE, compress_bound  # noqa: F401  (re-exported)

CHECKSUM, SPLIT, FSE_TABLES = 1, 4, 16
S, W = 128 << 10, 8 << 10              # the emulator build's segment and overlap (checked against what the binary reports)


def build():
    return emu_common.build("emu_encode_fse")


def run(buffers, caps=None, flags=FSE_TABLES, timeout=900):
    """[(result record, whole output region — 0xEE where nothing was written)] per buffer."""
    caps = emu_common.compress_caps(buffers, caps)
    (raw,), _ = emu_common.execute("emu_encode_fse", emu_common.compress_batch(buffers, caps, flags), timeout)
    assert struct.unpack_from("<QQ", raw, 0) == (S, W)
    return emu_common.results(raw, 16, COMPRESS_RESULT_DTYPE, caps)
