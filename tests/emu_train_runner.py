"""Runs dictionary training (the cz_train_*_kernel launches of cz_dictionary_train_device, the unmodified kernel sources) on the
CPU SIMT emulator: tests/emu/emu_train.cpp, built by tests/emu/Makefile under ASan/UBSan.  Test infrastructure only."""
import struct

import emu_common
from emu_common import EMU_DIR  # noqa: F401  (re-exported)

INVALID_ARG = 901


def build():
    return emu_common.build("emu_train")


def run(samples, capacity, dict_id=0, segment_len=0, reserved=(0,) * 6, params=True, claimed=None, timeout=1800):
    """(status, pieces, dict_len, the whole output region — 0xEE where nothing was written).  params=False: the kernel's host is
    given no parameters.  claimed: lengths to announce instead of the samples' own (for the checks that only read lengths)."""
    batch = struct.pack("<QQI", len(samples), capacity, 1 if params else 0) + struct.pack("<8I", dict_id, segment_len, *reserved)
    batch += b"".join(struct.pack("<QQ", len(b) if claimed is None else claimed[i], len(b)) + bytes(b) for i, b in enumerate(samples))
    (raw,), _ = emu_common.execute("emu_train", batch, timeout)
    status, pieces, n = struct.unpack_from("<iIQ", raw, 0)
    return status, pieces, n, raw[16:16 + capacity]


def train(samples, capacity, **kw):
    """The dictionary (bytes); the checks every run must pass are made here."""
    status, _, n, region = run(samples, capacity, **kw)
    assert status == 0, status
    assert 0 < n <= capacity
    assert set(region[n:]) <= {0xEE}, "bytes past dict_len were touched"
    return region[:n]
