"""Runs the several-dictionaries batch path (cz_context_set_dictionaries) on the CPU SIMT emulator: tests/emu/emu_multidict.cpp,
built by tests/emu/Makefile under ASan/UBSan.  Test infrastructure only."""
import emu_common
from emu_common import EMU_DIR, RESULT_DTYPE  # noqa: F401  (re-exported)


def build():
    return emu_common.build("emu_multidict")


def run(frames, caps, dicts, no_id=None, chain_bytes=0, lit_bytes=0, verify=True, timeout=900):
    """[(result record, whole output region — 0xEE where nothing was written)] per frame; `dicts`: files of the registered
    dictionaries, `no_id`: file of the no-ID dictionary or None."""
    raw, run.last_stderr = emu_common.execute("emu_multidict", emu_common.decode_batch(frames, caps), timeout,
                                              EMU_CHAIN=str(int(chain_bytes)), EMU_LIT=str(int(lit_bytes)), EMU_VERIFY="1" if verify else "0",
                                              EMU_DICTS=":".join(dicts), EMU_DUMP_ALL="1", EMU_NOID_DICT=no_id or None)
    return emu_common.results(raw[0], 0, RESULT_DTYPE, caps)
