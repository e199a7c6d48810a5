"""Time of dictionary training on the device (cz_dictionary_train_device) next to libzstd's ZDICT_trainFromBuffer on the same box.

Run it on the GPU box under a time limit of its own, e.g.
    timeout -k 10 900 python scripts/train_bench.py --out profiles/compress/train_bench.json
Samples: the --records records of scripts/compress_dict_bench.py (dict_records.records(records / 4, seed=1)), one training per
family and capacity (8 KiB and 112 KiB).  Device: the samples already in HBM; kernel_ms is the sum of the four steps' device times
(cz_dictionary_train_last_ms: frequencies, epochs, statistics, tables), wall_ms the whole call, the median of --runs after one
warm-up.  ZDICT: one call on one CPU thread, wall time.  A last row gives the size of the tests' 800 held-out records under this
library's compressor with dictionaries trained here on 600 records per family (T), with the golden ZDICT dictionaries (Z) and
without (P).  Prints one JSON line per row and writes them to --out."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dict_records as dr  # noqa: E402
import train_data as td  # noqa: E402


def device_train(cz, ctx, samples, capacity, runs):
    import torch
    dev = torch.device("cuda:0")
    lens = np.array([len(b) for b in samples], dtype=np.uint64)
    off = np.zeros(len(samples), dtype=np.uint64)
    off[1:] = np.cumsum(lens[:-1])
    d_in = torch.from_numpy(np.frombuffer(b"".join(samples) + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
    desc = torch.from_numpy(np.stack([off, lens]).view(np.int64)).to(dev)
    d_out = torch.zeros(capacity, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    wall, steps, n = [], [], 0
    for r in range(runs + 1):
        t = time.perf_counter()
        n = ctx.train_dictionary_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(samples), d_out.data_ptr(), capacity)
        dt = (time.perf_counter() - t) * 1e3
        if r:
            wall.append(dt)
            steps.append(ctx.last_train_ms())
    steps = np.median(np.array(steps), axis=0)
    return float(np.median(wall)), [float(x) for x in steps], d_out.cpu().numpy()[:n].tobytes()


def zdict_train(samples, capacity):
    try:
        z = ctypes.CDLL("libzstd.so.1")
        z.ZDICT_trainFromBuffer.restype = ctypes.c_size_t
        z.ZDICT_trainFromBuffer.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint]
        z.ZDICT_isError.restype = ctypes.c_uint
        z.ZDICT_isError.argtypes = [ctypes.c_size_t]
        z.ZSTD_versionNumber.restype = ctypes.c_uint
    except (OSError, AttributeError):
        return None
    blob = b"".join(samples)
    sizes = (ctypes.c_size_t * len(samples))(*[len(b) for b in samples])
    out = ctypes.create_string_buffer(capacity)
    t = time.perf_counter()
    n = z.ZDICT_trainFromBuffer(out, capacity, blob, sizes, len(samples))
    dt = (time.perf_counter() - t) * 1e3
    if z.ZDICT_isError(n):
        return None
    return dt, out.raw[:n], z.ZSTD_versionNumber()


def held_out_sizes(cz, ctx):
    held = dr.records(200, seed=7)
    bufs, idx = [b for _, b in held], [j for j, _ in held]
    sizes = {}
    for name, raws in (("T", [cz.train_dictionary(td.family_records(j, 600), 8192, ctx) for j in range(4)]), ("Z", dr.dictionaries())):
        ctx.set_compress_dictionaries([cz.Dictionary(ctx, raw) for raw in raws])
        sizes[name] = sum(len(f) for _, f in cz.compress_batch_host_dict(bufs, idx, ctx))
    sizes["P"] = sum(len(f) for _, f in cz.compress_batch_host(bufs, ctx))
    return dict(row="held_out_800_records", T=sizes["T"], Z=sizes["Z"], P=sizes["P"], T_over_P=round(sizes["T"] / sizes["P"], 4),
                Z_over_P=round(sizes["Z"] / sizes["P"], 4), T_over_Z=round(sizes["T"] / sizes["Z"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-zdict", action="store_true")
    args = ap.parse_args()
    import torch
    import cairo_zstd_amd as cz
    recs = dr.records(args.records // 4, seed=1)
    ctx = cz.Context(0)
    rows = []
    for j, (fam, _) in enumerate(dr.FAMILIES):
        samples = [b for k, b in recs if k == j]
        nbytes = sum(len(b) for b in samples)
        for capacity in (8 << 10, 112 << 10):
            wall, steps, raw = device_train(cz, ctx, samples, capacity, args.runs)
            row = dict(family=fam, samples=len(samples), sample_bytes=nbytes, capacity=capacity, device=torch.cuda.get_device_name(0),
                       dict_len=len(raw), device_wall_ms=round(wall, 3), device_kernel_ms=round(sum(steps), 3),
                       device_step_ms=dict(zip(("frequencies", "epochs", "statistics", "tables"), (round(x, 3) for x in steps))))
            ref = None if args.no_zdict else zdict_train(samples, capacity)
            if ref:
                row.update(zdict_wall_ms=round(ref[0], 3), zdict_len=len(ref[1]), libzstd_version=ref[2], zdict_threads=1)
            print(json.dumps(row), flush=True)
            rows.append(row)
    row = held_out_sizes(cz, ctx)
    print(json.dumps(row), flush=True)
    rows.append(row)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
