"""Writes tests/golden/compress_records/manifest.json: the sha256 of every frame the records level (CZ_COMPRESS_RECORDS) writes for
records_edges.manifest_batch() with the four family dictionaries, under flags 64, 65, 66 and 67, as the CPU emulator of the
unmodified kernel (tests/emu/emu_encode_records.cpp) computes them.  The GPU tests check the device's frames against it."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import dict_records as dr  # noqa: E402
import emu_encode_records_runner as emu  # noqa: E402
import records_edges as rede  # noqa: E402


def main():
    bufs, idx = rede.manifest_batch()
    out = {"dictionaries": [name for _, name in dr.FAMILIES], "n": len(bufs), "flags": {}}
    for flags in (emu.RECORDS, emu.RECORDS | emu.CHECKSUM, emu.RECORDS | emu.NO_DICT_ID, emu.RECORDS | emu.CHECKSUM | emu.NO_DICT_ID):
        got = emu.run(bufs, dr.dictionaries(), index=idx, flags=flags)
        assert all(int(r["status"]) == 0 for r, _ in got)
        out["flags"][str(flags)] = [hashlib.sha256(region[:int(r["bytes_written"])]).hexdigest() for r, region in got]
    path = os.path.join(ROOT, "tests", "golden", "compress_records", "manifest.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    main()
