"""Writes tests/golden/train/manifest.json: the sha256 and length of the dictionary that training makes of every input of
train_data.manifest_inputs(), as the CPU emulator of the unmodified kernels (tests/emu/emu_train.cpp) computes it.  The GPU tests
check the device's dictionaries against it."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import emu_train_runner as emu  # noqa: E402
import train_data as td  # noqa: E402


def main():
    out = {}
    for name, (samples, cap) in sorted(td.manifest_inputs().items()):
        raw = emu.train(samples, cap)
        out[name] = {"samples": len(samples), "capacity": cap, "len": len(raw), "sha256": hashlib.sha256(raw).hexdigest()}
    path = os.path.join(ROOT, "tests", "golden", "train", "manifest.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    main()
