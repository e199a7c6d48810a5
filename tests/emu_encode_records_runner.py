"""Runs the records level (CZ_COMPRESS_RECORDS: cz_compress_records_kernel, cz_compress_records_dict_kernel, behind
cz_dict_setup_kernel and cz_enc_dict_prep_kernel for the dictionaries) on the CPU SIMT emulator: tests/emu/emu_encode_records.cpp,
built by tests/emu/Makefile.encode_records under ASan/UBSan.  Test infrastructure only."""
import fcntl
import os
import struct
import subprocess
import tempfile

import numpy as np

from emu_encode_runner import COMPRESS_RESULT_DTYPE, CHECKSUM, compress_bound  # noqa: F401  (re-exported)

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
NO_DICT = 0xFFFFFFFF
NO_DICT_ID = 2
RECORDS = 64
RECORD_MAX = 32 << 10                 # cz_compress_record_max (checked against what the binary reports)


def build():
    with open(os.path.join(EMU_DIR, ".emu_encode_records.lock"), "w") as lk:     # several test workers may ask at once
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", EMU_DIR, "-f", "Makefile.encode_records", "emu_encode_records"], stdout=subprocess.DEVNULL)
    return os.path.join(EMU_DIR, "emu_encode_records")


def run(buffers, dicts=None, index=None, caps=None, flags=RECORDS, timeout=1800):
    """[(result record, whole output region — 0xEE where nothing was written)] per buffer.  dicts=None: the kernel without
    dictionaries (cz_compress_batch_device); else the dictionary kernel with these raw dictionaries (bytes) and index: one entry
    per buffer (NO_DICT: none) or None (the kernel is given no index: every frame uses dicts[0])."""
    exe = build()
    caps = [compress_bound(len(b)) for b in buffers] if caps is None else list(caps)
    mode = 0 if dicts is None else (1 if index is None else 2)
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<QII", len(buffers), flags, len(dicts or [])))
            for d in dicts or []:
                f.write(struct.pack("<Q", len(d)))
                f.write(bytes(d))
            f.write(struct.pack("<I", mode))
            for i, (b, cap) in enumerate(zip(buffers, caps)):
                f.write(struct.pack("<QQI", len(b), cap, 0 if index is None else index[i]))
                f.write(bytes(b))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        p = subprocess.run([exe, inp, outp], capture_output=True, timeout=timeout, env=env)
        if p.returncode != 0:
            raise RuntimeError(f"emu_encode_records failed rc={p.returncode}\n{p.stderr.decode()[-4000:]}")
        raw = open(outp, "rb").read()
    assert struct.unpack_from("<Q", raw, 0) == (RECORD_MAX,)
    out, pos = [], 8
    for cap in caps:
        r = np.frombuffer(raw, dtype=COMPRESS_RESULT_DTYPE, count=1, offset=pos)[0]
        pos += COMPRESS_RESULT_DTYPE.itemsize
        out.append((r, raw[pos:pos + cap]))
        pos += cap
    return out
