"""Writes tests/golden/compress_dict_edges/manifest.json: the sha256 of every frame the dictionary compressor writes for the edge
inputs of tests/dict_edges.py that the CPU emulator takes, each against its hand-built dictionary, under flags 0 and under
CZ_COMPRESS_CHECKSUM, as the CPU emulator of the unmodified kernels (tests/emu/emu_encode_dict.cpp) computes them.  The GPU tests
check the device's frames against it."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import dict_edges as de  # noqa: E402
import emu_encode_dict_runner as emu  # noqa: E402


def main():
    edges = [e for e in de.edges() if e.emu]
    bufs, dicts, idx = de.batch(edges)
    out = {"names": [e.name for e in edges], "flags": {}}
    for flags in (0, emu.CHECKSUM):
        got = emu.run(bufs, dicts, index=idx, flags=flags)
        assert all(int(r["status"]) == 0 for r, _ in got)
        out["flags"][str(flags)] = [hashlib.sha256(region[:int(r["bytes_written"])]).hexdigest() for r, region in got]
    path = os.path.join(ROOT, "tests", "golden", "compress_dict_edges", "manifest.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    main()
