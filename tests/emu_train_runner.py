"""Runs dictionary training (the cz_train_*_kernel launches of cz_dictionary_train_device, the unmodified kernel sources) on the
CPU SIMT emulator: tests/emu/emu_train.cpp, built by tests/emu/Makefile.train under ASan/UBSan.  Test infrastructure only."""
import fcntl
import os
import struct
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
INVALID_ARG = 901


def build():
    with open(os.path.join(EMU_DIR, ".emu_train.lock"), "w") as lk:         # several test workers may ask at once
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", EMU_DIR, "-f", "Makefile.train", "emu_train"], stdout=subprocess.DEVNULL)
    return os.path.join(EMU_DIR, "emu_train")


def run(samples, capacity, dict_id=0, segment_len=0, reserved=(0,) * 6, params=True, claimed=None, timeout=1800):
    """(status, pieces, dict_len, the whole output region — 0xEE where nothing was written).  params=False: the kernel's host is
    given no parameters.  claimed: lengths to announce instead of the samples' own (for the checks that only read lengths)."""
    exe = build()
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<QQI", len(samples), capacity, 1 if params else 0))
            f.write(struct.pack("<8I", dict_id, segment_len, *reserved))
            for i, b in enumerate(samples):
                f.write(struct.pack("<QQ", len(b) if claimed is None else claimed[i], len(b)))
                f.write(bytes(b))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        p = subprocess.run([exe, inp, outp], capture_output=True, timeout=timeout, env=env)
        if p.returncode != 0:
            raise RuntimeError(f"emu_train failed rc={p.returncode}\n{p.stderr.decode()[-4000:]}")
        raw = open(outp, "rb").read()
    status, pieces, n = struct.unpack_from("<iIQ", raw, 0)
    return status, pieces, n, raw[16:16 + capacity]


def train(samples, capacity, **kw):
    """The dictionary (bytes); the checks every run must pass are made here."""
    status, _, n, region = run(samples, capacity, **kw)
    assert status == 0, status
    assert 0 < n <= capacity
    assert set(region[n:]) <= {0xEE}, "bytes past dict_len were touched"
    return region[:n]
