"""Runs the several-dictionaries batch path (cz_context_set_dictionaries) on the CPU SIMT emulator: tests/emu/emu_multidict.cpp,
built by tests/emu/Makefile.multidict under ASan/UBSan.  Test infrastructure only."""
import fcntl
import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
RESULT_DTYPE = np.dtype([("status", "<i4"), ("blocks_decoded", "<u4"), ("bytes_consumed", "<u8"),
                         ("bytes_produced", "<u8"), ("checksum_from_data", "<u4"), ("flags", "<u4"),
                         ("detail", "<u8", (2,)), ("calculated_checksum", "<u4"), ("reserved", "<u4")])


def build():
    with open(os.path.join(EMU_DIR, ".emu_multidict.lock"), "w") as lk:      # several test workers may ask at once
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", EMU_DIR, "-f", "Makefile.multidict", "emu_multidict"], stdout=subprocess.DEVNULL)
    return os.path.join(EMU_DIR, "emu_multidict")


def run(frames, caps, dicts, no_id=None, chain_bytes=0, lit_bytes=0, verify=True, timeout=900):
    """[(result record, whole output region — 0xEE where nothing was written)] per frame; `dicts`: files of the registered
    dictionaries, `no_id`: file of the no-ID dictionary or None."""
    exe = build()
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<Q", len(frames)))
            for fr, cap in zip(frames, caps):
                f.write(struct.pack("<QQ", len(fr), cap))
                f.write(fr)
        env = dict(os.environ, EMU_CHAIN=str(int(chain_bytes)), EMU_LIT=str(int(lit_bytes)), EMU_VERIFY="1" if verify else "0",
                   EMU_DICTS=":".join(dicts), EMU_DUMP_ALL="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
                   UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        env.pop("EMU_NOID_DICT", None)
        if no_id:
            env["EMU_NOID_DICT"] = no_id
        p = subprocess.run([exe, inp, outp], capture_output=True, timeout=timeout, env=env)
        run.last_stderr = p.stderr.decode()[-2000:]
        if p.returncode != 0:
            raise RuntimeError(f"emu_multidict failed rc={p.returncode}\n{p.stderr.decode()[-4000:]}")
        raw = open(outp, "rb").read()
    out, pos = [], 0
    for cap in caps:
        r = np.frombuffer(raw, dtype=RESULT_DTYPE, count=1, offset=pos)[0]
        pos += RESULT_DTYPE.itemsize
        out.append((r, raw[pos:pos + cap]))
        pos += cap
    return out
