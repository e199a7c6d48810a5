"""Runs the dictionary compressor (cz_dict_setup_kernel, cz_enc_dict_prep_kernel, cz_compress_frames_dict_kernel) on the CPU
SIMT emulator: tests/emu/emu_encode_dict.cpp, built by tests/emu/Makefile under ASan/UBSan.  Test infrastructure only."""
import numpy as np

import emu_common
from emu_common import EMU_DIR, COMPRESS_RESULT_DTYPE, compress_bound  # noqa: F401  (re-exported)
from emu_encode_runner import CHECKSUM  # noqa: F401  (re-exported)

NO_DICT = 0xFFFFFFFF
NO_DICT_ID = 2


def build():
    return emu_common.build("emu_encode_dict")


def run(buffers, dicts, index=None, caps=None, flags=0, timeout=1800, tables=False):
    """[(result record, whole output region — 0xEE where nothing was written)] per buffer.  dicts: raw dictionaries (bytes);
    index: one entry per buffer (NO_DICT: none) or None (the kernel is given no index: every frame uses dicts[0]).
    tables=True: (that list, [the prepared hash table of each dictionary, 2^14 uint32])."""
    caps = emu_common.compress_caps(buffers, caps)
    batch = emu_common.compress_batch(buffers, caps, flags, dicts=list(dicts), mode=0 if index is None else 1, index=index)
    (raw, *tabs), _ = emu_common.execute("emu_encode_dict", batch, timeout, outputs=2 if tables else 1)
    out = emu_common.results(raw, 0, COMPRESS_RESULT_DTYPE, caps)
    return (out, list(np.frombuffer(tabs[0], dtype=np.uint32).reshape(len(dicts), 1 << 14))) if tables else out
