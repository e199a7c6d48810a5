"""Throughput and ratio of compression with dictionaries (cz_compress_batch_dict_device) on many small records, next to the same
records without dictionaries and to libzstd level 1 with a ZSTD_CDict per dictionary on 16 CPU threads.

Run it on the GPU box under a time limit of its own, e.g.
    timeout -k 10 900 python scripts/compress_dict_bench.py --out profiles/compress/dict_bench.json
The batch: --records records (110-420 bytes) of the four families of tests/dict_records.py, interleaved, each with its family's
dictionary (tests/golden/multidict/dict_{a,b,c,d}.bin).  The device figure is input bytes over the kernel time (hipEvents around
the launch, median of --runs after one warm-up), buffers already in HBM.  Prints one JSON line per configuration and writes them to
--out."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dict_records as dr  # noqa: E402

NO_DICT = 0xFFFFFFFF


def device_run(cz, ctx, stream, bufs, idx, runs):
    """(median kernel ms, frame bytes); idx None: the plain compressor."""
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
    d_idx = torch.from_numpy(np.array(idx, dtype=np.uint32).view(np.int32)).to(dev) if idx is not None else None
    d_res = torch.zeros(len(bufs) * 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    times = []
    for r in range(runs + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        if idx is None:
            ctx.compress_batch_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(bufs), d_out.data_ptr(),
                                      desc[2].data_ptr(), desc[3].data_ptr(), d_res.data_ptr())
        else:
            ctx.compress_batch_dict_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(bufs), d_out.data_ptr(),
                                           desc[2].data_ptr(), desc[3].data_ptr(), d_idx.data_ptr(), d_res.data_ptr())
        e1.record(stream)
        e1.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    res = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)
    assert (res["status"] == 0).all()
    return float(np.median(times)), int(res["bytes_written"].sum())


def libzstd_run(bufs, idx, dicts, threads, runs):
    try:
        z = ctypes.CDLL("libzstd.so.1")
    except OSError:
        return None
    z.ZSTD_compressBound.restype = ctypes.c_size_t
    z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    z.ZSTD_createCDict.restype = ctypes.c_void_p
    z.ZSTD_createCDict.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    z.ZSTD_createCCtx.restype = ctypes.c_void_p
    z.ZSTD_compress_usingCDict.restype = ctypes.c_size_t
    z.ZSTD_compress_usingCDict.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    z.ZSTD_versionNumber.restype = ctypes.c_uint
    cdicts = [z.ZSTD_createCDict(d, len(d), 1) for d in dicts]
    outs = [ctypes.create_string_buffer(z.ZSTD_compressBound(len(b))) for b in bufs]
    n = len(bufs)
    per = (n + threads - 1) // threads

    def part(k):                                                        # one context per thread, its share of the records
        cctx, total = z.ZSTD_createCCtx(), 0
        for i in range(k * per, min(n, (k + 1) * per)):
            total += z.ZSTD_compress_usingCDict(cctx, outs[i], len(outs[i]), bufs[i], len(bufs[i]), cdicts[idx[i]])
        return total
    best, total = None, 0
    with ThreadPoolExecutor(threads) as ex:
        for _ in range(runs):
            t = time.perf_counter()
            total = sum(ex.map(part, range(threads)))
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
    return best * 1e3, total, z.ZSTD_versionNumber()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    import torch
    import cairo_zstd_amd as cz
    recs = dr.records(args.records // 4, seed=1)
    bufs, idx = [b for _, b in recs], [j for j, _ in recs]
    raw = dr.dictionaries()
    nbytes = sum(len(b) for b in bufs)
    stream = torch.cuda.Stream()
    ctx = cz.Context(0, stream.cuda_stream)
    ctx.set_compress_dictionaries([cz.Dictionary(ctx, d) for d in raw])
    rows = []
    for name, ix in (("with_dictionaries", idx), ("without", None)):
        ms, written = device_run(cz, ctx, stream, bufs, ix, args.runs)
        row = dict(batch=f"{len(bufs)} records", mode=name, input_bytes=nbytes, device=torch.cuda.get_device_name(0), device_ms=round(ms, 3),
                   device_gbps=round(nbytes / ms / 1e6, 3), device_ratio=round(nbytes / written, 4), device_bytes=written)
        if ix is not None:
            cpu = libzstd_run(bufs, idx, raw, args.threads, args.runs)
            if cpu:
                cms, cwritten, ver = cpu
                row.update(libzstd_version=ver, libzstd_level=1, libzstd_cdict=True, libzstd_threads=args.threads, libzstd_ms=round(cms, 3),
                           libzstd_gbps=round(nbytes / cms / 1e6, 3), libzstd_ratio=round(nbytes / cwritten, 4), libzstd_bytes=cwritten)
        print(json.dumps(row), flush=True)
        rows.append(row)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
