"""Throughput and ratio of the batched compressor (cz_compress_batch_device) next to libzstd level 1 on 16 CPU threads.

Run it on the GPU box under a time limit of its own, e.g.
    timeout -k 10 600 python scripts/compress_bench.py --out profiles/compress/bench.json
Three batches tiled from the golden corpus originals (tests/golden/decode_corpus): 10 000 x 128 KiB, 64 x 2 MiB and 1 x 16 MiB.
The device figure is input bytes over the kernel time (hipEvents around the launch, median of --runs after one warm-up), buffers
already in HBM.  libzstd (ZSTD_compress, level 1, dlopen'ed) runs the same buffers on --threads threads; it is skipped when the
host has no libzstd.so.1 or with --no-libzstd.  Prints one JSON line per batch and writes them all to --out.

--split compresses with CZ_COMPRESS_SPLIT.  --pieces adds the frame bytes of every 128 KiB piece of the 64 x 2 MiB
batch compressed as a frame of its own, the floor the choice of segment and overlap is judged against.  Builds with another segment
or overlap (make -C cairo_zstd_amd/csrc exp NAME=s2w128 EXPFLAGS="-DCZE_SEG_BLOCKS=2u -DCZE_OVERLAP=131072u") are picked with
CAIRO_ZSTD_AMD_LIB; --tag goes into every row to tell them apart.

--high measures CZ_COMPRESS_HIGH next to CZ_COMPRESS_FSE_TABLES and libzstd levels 1, 3 and 6 (DESIGN.md §10.8;
profiles/compress/high_bench.json).
--high-split measures CZ_COMPRESS_HIGH_SPLIT next to CZ_COMPRESS_HIGH and CZ_COMPRESS_SPLIT | CZ_COMPRESS_FSE_TABLES in one session, with
the fastest and slowest run of each, and libzstd levels 3 and 6 (profiles/compress/high_split_bench.json).
--fse-tables measures CZ_COMPRESS_FSE_TABLES: every batch unsplit and split, each without and with the flag in
the same session, and the frame bytes of the 69 corpus originals without and with it; --out defaults to
profiles/compress/fse_bench.json."""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def corpus_pool():
    d = os.path.join(ROOT, "tests", "golden", "decode_corpus")
    return b"".join(open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if not n.endswith(".zst"))


def tiled(n, size, seed):
    pool = corpus_pool()
    pool = pool * (size // len(pool) + 2)
    starts = np.random.default_rng(seed).integers(0, len(pool) - size, n)
    return [pool[int(s):int(s) + size] for s in starts]


def device_run(cz, ctx, stream, bufs, runs, split=False, fse=False, high=False, high_split=False, spread=False):
    """(median ms of `runs` launches after one warm-up, frame bytes); with `spread` also the fastest and the slowest run."""
    import torch
    dev = torch.device("cuda:0")
    lens = np.array([len(b) for b in bufs], dtype=np.uint64)
    in_off = np.zeros(len(bufs), dtype=np.uint64)
    in_off[1:] = np.cumsum(lens[:-1])
    caps = np.array([cz.compress_bound(int(l)) for l in lens], dtype=np.uint64)
    out_off = np.zeros(len(bufs), dtype=np.uint64)
    out_off[1:] = np.cumsum(caps[:-1])
    d_in = torch.from_numpy(np.frombuffer(b"".join(bufs), dtype=np.uint8).copy()).to(dev)
    d_out = torch.empty(int(caps.sum()), dtype=torch.uint8, device=dev)
    desc = torch.from_numpy(np.stack([in_off, lens, out_off, caps]).view(np.int64)).to(dev)
    d_res = torch.zeros(len(bufs) * 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    times = []
    for r in range(runs + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ctx.compress_batch_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(bufs), d_out.data_ptr(),
                                  desc[2].data_ptr(), desc[3].data_ptr(), d_res.data_ptr(), **(dict(split=True) if split else {}),
                                  **(dict(fse_tables=True) if fse else {}), **(dict(high=True) if high else {}),
                                  **(dict(high_split=True) if high_split else {}))
        e1.record(stream)
        e1.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    res = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)
    assert (res["status"] == 0).all()
    if spread:
        return float(np.median(times)), int(res["bytes_written"].sum()), float(min(times)), float(max(times))
    return float(np.median(times)), int(res["bytes_written"].sum())


def libzstd_run(bufs, threads, runs, level=1):
    try:
        z = ctypes.CDLL("libzstd.so.1")
    except OSError:
        return None
    z.ZSTD_compressBound.restype = ctypes.c_size_t
    z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    z.ZSTD_compress.restype = ctypes.c_size_t
    z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    z.ZSTD_versionNumber.restype = ctypes.c_uint
    outs = [ctypes.create_string_buffer(z.ZSTD_compressBound(len(b))) for b in bufs]

    def one(i):
        return z.ZSTD_compress(outs[i], len(outs[i]), bufs[i], len(bufs[i]), level)     # ctypes drops the GIL around the call
    best, total = None, 0
    with ThreadPoolExecutor(threads) as ex:
        for _ in range(runs):
            t = time.perf_counter()
            sizes = list(ex.map(one, range(len(bufs)), chunksize=max(1, len(bufs) // (threads * 8))))
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
            total = sum(sizes)
    return best * 1e3, total, z.ZSTD_versionNumber()


def high_bench(args, cz, ctx, stream, device):
    """CZ_COMPRESS_FSE_TABLES and CZ_COMPRESS_HIGH in one session: frame bytes of the corpus originals, kernel time (median of
    --runs after a warm-up) and ratio on 10 000 x 128 KiB and 64 x 2 MiB, libzstd levels 1, 3 and 6 on --threads CPUs."""
    out = args.out or os.path.join(ROOT, "profiles", "compress", "high_bench.json")
    d = os.path.join(ROOT, "tests", "golden", "decode_corpus")
    originals = [open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if not n.endswith(".zst")]
    row = dict(batch="corpus originals", count=len(originals), input_bytes=sum(map(len, originals)))
    row["frame_bytes_fse_tables"] = sum(len(fr) for _, fr in cz.compress_batch_host(originals, ctx, fse_tables=True))
    row["frame_bytes_high"] = sum(len(fr) for _, fr in cz.compress_batch_host(originals, ctx, high=True))
    for level in (() if args.no_libzstd else (1, 3, 6)):
        cpu = libzstd_run(originals, args.threads, 1, level)
        if cpu:
            row[f"libzstd_{level}_frame_bytes"] = cpu[1]
    rows = [row]
    print(json.dumps(row), flush=True)
    for name, n, size in (("10000x128KiB", 10000, 128 << 10), ("64x2MiB", 64, 2 << 20)):
        bufs = tiled(n, size, seed=1)
        nbytes = n * size
        row = dict(batch=name, input_bytes=nbytes, device=device)
        for key, kw in (("fse_tables", dict(fse=True)), ("high", dict(high=True)), ("fse_tables_again", dict(fse=True))):
            ms, written = device_run(cz, ctx, stream, bufs, args.runs, **kw)
            row[key] = dict(device_ms=round(ms, 3), device_gbps=round(nbytes / ms / 1e6, 2), device_ratio=round(nbytes / written, 4), frame_bytes=written)
        for level in (() if args.no_libzstd else (1, 3, 6)):
            cpu = libzstd_run(bufs, args.threads, args.runs, level)
            if cpu:
                row[f"libzstd_{level}"] = dict(threads=args.threads, ms=round(cpu[0], 3), gbps=round(nbytes / cpu[0] / 1e6, 2), ratio=round(nbytes / cpu[1], 4))
        if args.tag:
            row["tag"] = args.tag
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rows, f, indent=1)


def high_split_bench(args, cz, ctx, stream, device):
    """CZ_COMPRESS_HIGH, CZ_COMPRESS_HIGH_SPLIT and CZ_COMPRESS_SPLIT | CZ_COMPRESS_FSE_TABLES in one session on 64 x 2 MiB, 1 x 16 MiB and
    10 000 x 128 KiB: kernel time (median, fastest and slowest of --runs after a warm-up) and frame bytes; libzstd levels 3 and 6 on
    --threads CPUs.  Every row says how much faster the split form is and whether its slowest run is below the unsplit form's fastest."""
    out = args.out or os.path.join(ROOT, "profiles", "compress", "high_split_bench.json")
    rows = []
    for name, n, size in (("64x2MiB", 64, 2 << 20), ("1x16MiB", 1, 16 << 20), ("10000x128KiB", 10000, 128 << 10)):
        bufs = tiled(n, size, seed=1)
        nbytes = n * size
        row = dict(batch=name, input_bytes=nbytes, device=device, runs=args.runs, segment=cz.compress_split_segment())
        for key, kw in (("high", dict(high=True)), ("high_split", dict(high_split=True)), ("split_fse_tables", dict(split=True, fse=True)),
                        ("high_again", dict(high=True))):
            ms, written, lo, hi = device_run(cz, ctx, stream, bufs, args.runs, spread=True, **kw)
            row[key] = dict(device_ms=round(ms, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), device_gbps=round(nbytes / ms / 1e6, 2),
                            device_ratio=round(nbytes / written, 4), frame_bytes=written)
        h_lo = min(row["high"]["min_ms"], row["high_again"]["min_ms"])
        h_hi = max(row["high"]["max_ms"], row["high_again"]["max_ms"])
        row["high_over_high_split"] = round(row["high"]["device_ms"] / row["high_split"]["device_ms"], 3)
        row["high_split_slowest_below_high_fastest"] = row["high_split"]["max_ms"] < h_lo
        row["high_split_within_high_spread"] = h_lo <= row["high_split"]["device_ms"] <= h_hi
        for level in (() if args.no_libzstd else (3, 6)):
            cpu = libzstd_run(bufs, args.threads, args.runs, level)
            if cpu:
                row[f"libzstd_{level}"] = dict(threads=args.threads, ms=round(cpu[0], 3), gbps=round(nbytes / cpu[0] / 1e6, 2), ratio=round(nbytes / cpu[1], 4),
                                               frame_bytes=cpu[1])
        if args.tag:
            row["tag"] = args.tag
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--split", action="store_true", help="compress with CZ_COMPRESS_SPLIT")
    ap.add_argument("--pieces", action="store_true", help="also: the 64 x 2 MiB batch as 1 024 frames of 128 KiB (frame bytes)")
    ap.add_argument("--fse-tables", action="store_true", help="measure CZ_COMPRESS_FSE_TABLES next to the same launches without it")
    ap.add_argument("--high", action="store_true", help="measure CZ_COMPRESS_HIGH next to CZ_COMPRESS_FSE_TABLES, and libzstd levels 1, 3 and 6")
    ap.add_argument("--high-split", action="store_true", help="measure CZ_COMPRESS_HIGH_SPLIT next to CZ_COMPRESS_HIGH and CZ_COMPRESS_SPLIT | CZ_COMPRESS_FSE_TABLES")
    ap.add_argument("--no-libzstd", action="store_true")
    ap.add_argument("--tag", default=None, help="free text copied into every row")
    args = ap.parse_args()
    import torch
    import cairo_zstd_amd as cz
    stream = torch.cuda.Stream()                                        # the context launches on it, the events are recorded on it
    ctx = cz.Context(0, stream.cuda_stream)
    rows = []
    if args.fse_tables:
        args.out = args.out or os.path.join(ROOT, "profiles", "compress", "fse_bench.json")
        d = os.path.join(ROOT, "tests", "golden", "decode_corpus")
        originals = [open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if not n.endswith(".zst")]
        row = dict(batch="corpus originals", count=len(originals), input_bytes=sum(map(len, originals)))
        for key, fse in (("frame_bytes", False), ("frame_bytes_fse_tables", True)):
            row[key] = sum(len(fr) for _, fr in cz.compress_batch_host(originals, ctx, fse_tables=fse))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.high:
        high_bench(args, cz, ctx, stream, torch.cuda.get_device_name(0))
        ctx.close()
        return
    if args.high_split:
        high_split_bench(args, cz, ctx, stream, torch.cuda.get_device_name(0))
        ctx.close()
        return
    variants = [(s, f) for s in (False, True) for f in (False, True)] if args.fse_tables else [(args.split, False)]
    for name, n, size in (("10000x128KiB", 10000, 128 << 10), ("64x2MiB", 64, 2 << 20), ("1x16MiB", 1, 16 << 20)):
        bufs = tiled(n, size, seed=1)
        nbytes = n * size
        for split, fse in variants:
            ms, written = device_run(cz, ctx, stream, bufs, args.runs, split=split, fse=fse)
            row = dict(batch=name, input_bytes=nbytes, device=torch.cuda.get_device_name(0), device_ms=round(ms, 3),
                       device_gbps=round(nbytes / ms / 1e6, 2), device_ratio=round(nbytes / written, 4), frame_bytes=written, split=split)
            if args.fse_tables:
                row["fse_tables"] = fse
            if split:
                row["segment"] = cz.compress_split_segment()
            if args.tag:
                row["tag"] = args.tag
            if args.pieces and name == "64x2MiB":
                pieces = [b[o:o + (128 << 10)] for b in bufs for o in range(0, len(b), 128 << 10)]
                row["pieces_128KiB_frame_bytes"] = device_run(cz, ctx, stream, pieces, 1)[1]
            cpu = None if args.no_libzstd or (split, fse) != variants[0] else libzstd_run(bufs, args.threads, args.runs)
            if cpu:
                cms, cwritten, ver = cpu
                row.update(libzstd_version=ver, libzstd_level=1, libzstd_threads=args.threads, libzstd_ms=round(cms, 3),
                           libzstd_gbps=round(nbytes / cms / 1e6, 2), libzstd_ratio=round(nbytes / cwritten, 4))
            print(json.dumps(row), flush=True)
            rows.append(row)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
