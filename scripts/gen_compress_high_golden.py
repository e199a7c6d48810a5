#!/usr/bin/env python3
"""Writes tests/golden/compress_high/: the CZ_COMPRESS_HIGH frames the CPU emulator (tests/emu/emu_encode_high.cpp) makes of the
constructed inputs of tests/compress_high.py.  The frames of two_offsets, lazy_sites and two_blocks are kept whole (*.zst); the
manifest has the sha256 and length of every frame.  The device tests hold the MI355X to these bytes.  No GPU needed:
    python scripts/gen_compress_high_golden.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import compress_high as ch  # noqa: E402
import emu_encode_high_runner as emu  # noqa: E402

KEEP = ("two_offsets", "lazy_sites", "two_blocks")
OUT = os.path.join(ROOT, "tests", "golden", "compress_high")


def main():
    inputs = {k: b.data for k, (b, _) in ch.constructed().items()}
    inputs["two_blocks"] = ch.two_blocks().data
    inputs["raw_then_compressed"] = ch.raw_then_compressed().data
    os.makedirs(OUT, exist_ok=True)
    manifest = {"generator": "scripts/gen_compress_high_golden.py", "flags": emu.HIGH, "frames": {}}
    for (name, data), (r, region) in zip(inputs.items(), emu.run(list(inputs.values()), flags=emu.HIGH)):
        assert int(r["status"]) == 0, name
        frame = region[:int(r["bytes_written"])]
        manifest["frames"][name] = {"input_len": len(data), "input_sha256": hashlib.sha256(data).hexdigest(), "len": len(frame),
                                    "sha256": hashlib.sha256(frame).hexdigest(), "file": f"{name}.zst" if name in KEEP else None}
        if name in KEEP:
            with open(os.path.join(OUT, f"{name}.zst"), "wb") as f:
                f.write(frame)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
