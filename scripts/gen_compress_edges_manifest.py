"""Writes tests/golden/compress_edges/manifest.json: the sha256 of every frame the compressor writes for the edge inputs of
tests/compress_edges.py that the CPU emulator takes (emu_edges()), under flags 0 and under CZ_COMPRESS_CHECKSUM, as the CPU emulator
of the unmodified kernel (tests/emu/emu_encode.cpp) computes them.  The GPU tests check the device's frames against it."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import compress_edges as ce  # noqa: E402
import emu_encode_runner as emu  # noqa: E402


def main():
    edges = ce.emu_edges()
    out = {"names": [e.name for e in edges], "flags": {}}
    for flags in (0, emu.CHECKSUM):
        got = emu.run([e.data for e in edges], flags=flags)
        assert all(int(r["status"]) == 0 for r, _ in got)
        out["flags"][str(flags)] = [hashlib.sha256(region[:int(r["bytes_written"])]).hexdigest() for r, region in got]
    path = os.path.join(ROOT, "tests", "golden", "compress_edges", "manifest.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    main()
