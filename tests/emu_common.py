"""What the emulator runners (emu_runner, emu_*_runner) share: building a driver of tests/emu under ASan/UBSan (one Makefile, a
target per driver), running it on a batch file, and reading (result record, output region) pairs back.  Test infrastructure only."""
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
COMPRESS_RESULT_DTYPE = np.dtype([("status", "<i4"), ("blocks", "<u4"), ("bytes_read", "<u8"), ("bytes_written", "<u8"),
                                  ("checksum", "<u4"), ("flags", "<u4")])


def build(target):
    with open(os.path.join(EMU_DIR, f".{target}.lock"), "w") as lk:          # several test workers may ask at once
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", EMU_DIR, target], stdout=subprocess.DEVNULL)
    return os.path.join(EMU_DIR, target)


def execute(target, batch, timeout, outputs=1, **env):
    """Runs `target` on the bytes of a batch file: (the bytes of its `outputs` output files, the end of its stderr).  `env`: the
    driver's EMU_* settings (None: unset)."""
    exe = build(target)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", **env)
    env = {k: v for k, v in env.items() if v is not None}
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.bin"), [os.path.join(td, f"out{i}.bin") for i in range(outputs)]
        with open(inp, "wb") as f:
            f.write(batch)
        p = subprocess.run([exe, inp] + outp, capture_output=True, timeout=timeout, env=env)
        if p.returncode != 0:
            raise RuntimeError(f"{target} failed rc={p.returncode}\n{p.stderr.decode()[-4000:]}")
        return [open(o, "rb").read() for o in outp], p.stderr.decode()[-2000:]


def results(raw, pos, dtype, caps, produced=None):
    """[(result record, output region)] per cap from `pos` on; the region is the whole cap, or with `produced` what that field of
    the record says was written."""
    out = []
    for cap in caps:
        r = np.frombuffer(raw, dtype=dtype, count=1, offset=pos)[0]
        pos += dtype.itemsize
        w = min(int(r[produced]), cap) if produced else cap
        out.append((r, raw[pos:pos + w]))
        pos += w
    return out


def decode_batch(frames, caps):
    """batch.bin of the decode drivers"""
    return struct.pack("<Q", len(frames)) + b"".join(struct.pack("<QQ", len(fr), cap) + bytes(fr) for fr, cap in zip(frames, caps))


def compress_bound(n: int) -> int:
    """cz_compress_bound, restated (the emulator has no host library)."""
    blocks = (n + (128 << 10) - 1) // (128 << 10) if n else 1
    return 18 + 3 * blocks + n


def compress_caps(buffers, caps):
    return [compress_bound(len(b)) for b in buffers] if caps is None else list(caps)


def compress_batch(buffers, caps, flags, dicts=None, mode=0, index=None):
    """batch.bin of the encode drivers; with `dicts` (a list, possibly empty) that of the drivers with dictionaries: the
    dictionaries and a mode word after the header, a dict_index with every buffer."""
    if dicts is None:
        head = struct.pack("<QI", len(buffers), flags)
        return head + b"".join(struct.pack("<QQ", len(b), cap) + bytes(b) for b, cap in zip(buffers, caps))
    head = struct.pack("<QII", len(buffers), flags, len(dicts)) + b"".join(struct.pack("<Q", len(d)) + bytes(d) for d in dicts)
    return head + struct.pack("<I", mode) + b"".join(struct.pack("<QQI", len(b), cap, 0 if index is None else index[i]) + bytes(b)
                                                     for i, (b, cap) in enumerate(zip(buffers, caps)))
