"""Runs the records level (CZ_COMPRESS_RECORDS: cz_compress_records_kernel, cz_compress_records_dict_kernel, behind
cz_dict_setup_kernel and cz_enc_dict_prep_kernel for the dictionaries) on the CPU SIMT emulator: tests/emu/emu_encode_records.cpp,
built by tests/emu/Makefile under ASan/UBSan.  Test infrastructure only."""
import struct

import emu_common
from emu_common import EMU_DIR, COMPRESS_RESULT_DTYPE, compress_bound  # noqa: F401  (re-exported)
from emu_encode_runner import CHECKSUM  # noqa: F401  (re-exported)

NO_DICT = 0xFFFFFFFF
NO_DICT_ID = 2
RECORDS = 64
RECORD_MAX = 32 << 10                 # cz_compress_record_max (checked against what the binary reports)


def build():
    return emu_common.build("emu_encode_records")


def run(buffers, dicts=None, index=None, caps=None, flags=RECORDS, timeout=1800):
    """[(result record, whole output region — 0xEE where nothing was written)] per buffer.  dicts=None: the kernel without
    dictionaries (cz_compress_batch_device); else the dictionary kernel with these raw dictionaries (bytes) and index: one entry
    per buffer (NO_DICT: none) or None (the kernel is given no index: every frame uses dicts[0])."""
    caps = emu_common.compress_caps(buffers, caps)
    mode = 0 if dicts is None else (1 if index is None else 2)
    batch = emu_common.compress_batch(buffers, caps, flags, dicts=list(dicts or []), mode=mode, index=index)
    (raw,), _ = emu_common.execute("emu_encode_records", batch, timeout)
    assert struct.unpack_from("<Q", raw, 0) == (RECORD_MAX,)
    return emu_common.results(raw, 8, COMPRESS_RESULT_DTYPE, caps)
