"""Runs the dictionary compressor (cz_dict_setup_kernel, cz_enc_dict_prep_kernel, cz_compress_frames_dict_kernel) on the CPU
SIMT emulator: tests/emu/emu_encode_dict.cpp, built by tests/emu/Makefile.encode_dict under ASan/UBSan.  Test infrastructure only."""
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


def build():
    with open(os.path.join(EMU_DIR, ".emu_encode_dict.lock"), "w") as lk:     # several test workers may ask at once
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", EMU_DIR, "-f", "Makefile.encode_dict", "emu_encode_dict"], stdout=subprocess.DEVNULL)
    return os.path.join(EMU_DIR, "emu_encode_dict")


def run(buffers, dicts, index=None, caps=None, flags=0, timeout=1800, tables=False):
    """[(result record, whole output region — 0xEE where nothing was written)] per buffer.  dicts: raw dictionaries (bytes);
    index: one entry per buffer (NO_DICT: none) or None (the kernel is given no index: every frame uses dicts[0]).
    tables=True: (that list, [the prepared hash table of each dictionary, 2^14 uint32])."""
    exe = build()
    caps = [compress_bound(len(b)) for b in buffers] if caps is None else list(caps)
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<QII", len(buffers), flags, len(dicts)))
            for d in dicts:
                f.write(struct.pack("<Q", len(d)))
                f.write(bytes(d))
            f.write(struct.pack("<I", 0 if index is None else 1))
            for i, (b, cap) in enumerate(zip(buffers, caps)):
                f.write(struct.pack("<QQI", len(b), cap, 0 if index is None else index[i]))
                f.write(bytes(b))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        tabp = os.path.join(td, "tables.bin")
        p = subprocess.run([exe, inp, outp] + ([tabp] if tables else []), capture_output=True, timeout=timeout, env=env)
        if p.returncode != 0:
            raise RuntimeError(f"emu_encode_dict failed rc={p.returncode}\n{p.stderr.decode()[-4000:]}")
        raw = open(outp, "rb").read()
        tabs = np.fromfile(tabp, dtype=np.uint32).reshape(len(dicts), 1 << 14) if tables else None
    out, pos = [], 0
    for cap in caps:
        r = np.frombuffer(raw, dtype=COMPRESS_RESULT_DTYPE, count=1, offset=pos)[0]
        pos += COMPRESS_RESULT_DTYPE.itemsize
        out.append((r, raw[pos:pos + cap]))
        pos += cap
    return (out, list(tabs)) if tables else out
