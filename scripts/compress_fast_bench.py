"""Speed and ratio of the fast compression level (CZ_COMPRESS_FAST) next to the two existing configurations, flags 0
and CZ_COMPRESS_FSE_TABLES, measured in the same session on the same device.

Run it on the GPU box under a time limit of its own, e.g.
    timeout -k 10 600 python scripts/compress_fast_bench.py
The batches of scripts/compress_bench.py that are not one large buffer: 10 000 x 128 KiB and 64 x 2 MiB, tiled from the golden corpus
originals with the same seed.  Per batch the three configurations alternate (0, 16, 32, 0, 16, 32, ...) for --runs rounds after one
warm-up round; a row holds the median kernel time (hipEvents around the launch, inputs already in HBM), the fastest and slowest run,
input bytes over the median, and the ratio.  Every frame of the fast level is decoded by libzstd where the host has it (first 64
frames of a batch).  libzstd level 1 on --threads CPU threads runs the same buffers once per batch.  Prints one JSON line per row and
writes them all to --out (default profiles/compress/fast_bench.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import compress_frames as cf  # noqa: E402  (libzstd, dlopen'ed, to read frames back)
from compress_bench import libzstd_run, tiled  # noqa: E402

CONFIGS = (("flags 0", 0, {}), ("fse_tables", 16, dict(fse_tables=True)), ("fast", 32, dict(fast=True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compress", "fast_bench.json"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-libzstd", action="store_true")
    ap.add_argument("--tag", default=None, help="free text copied into every row")
    args = ap.parse_args()
    import torch
    import cairo_zstd_amd as cz
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()                                        # the context launches on it, the events are recorded on it
    ctx = cz.Context(0, stream.cuda_stream)
    rows = []
    for name, n, size in (("10000x128KiB", 10000, 128 << 10), ("64x2MiB", 64, 2 << 20)):
        bufs = tiled(n, size, seed=1)
        nbytes = n * size
        lens = np.full(n, size, dtype=np.uint64)
        in_off = np.arange(n, dtype=np.uint64) * np.uint64(size)
        caps = np.full(n, cz.compress_bound(size), dtype=np.uint64)
        out_off = np.arange(n, dtype=np.uint64) * caps[0]
        d_in = torch.from_numpy(np.frombuffer(b"".join(bufs), dtype=np.uint8).copy()).to(dev)
        d_out = torch.empty(int(caps.sum()), dtype=torch.uint8, device=dev)
        desc = torch.from_numpy(np.stack([in_off, lens, out_off, caps]).view(np.int64)).to(dev)
        d_res = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        times = {key: [] for key, _, _ in CONFIGS}
        written, blocks = {}, {}
        for r in range(args.runs + 1):
            for key, _, kw in CONFIGS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ctx.compress_batch_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), n, d_out.data_ptr(),
                                          desc[2].data_ptr(), desc[3].data_ptr(), d_res.data_ptr(), **kw)
                e1.record(stream)
                e1.synchronize()
                if r:
                    times[key].append(e0.elapsed_time(e1))
                    continue
                res = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)
                assert (res["status"] == 0).all(), key
                written[key], blocks[key] = int(res["bytes_written"].sum()), int(res["blocks"].sum())
                if key == "fast" and cf.libzstd():                      # the frames are real: libzstd reads them back
                    out = d_out[:64 * int(caps[0])].cpu().numpy()
                    for i in range(min(n, 64)):
                        o = int(out_off[i])
                        assert cf.libzstd_decompress(out[o:o + int(res[i]["bytes_written"])].tobytes(), size) == bufs[i], i
        cpu = None if args.no_libzstd else libzstd_run(bufs, args.threads, 3)
        for key, flags, _ in CONFIGS:
            ms = float(np.median(times[key]))
            row = dict(batch=name, config=key, flags=flags, input_bytes=nbytes, device=torch.cuda.get_device_name(0),
                       device_ms=round(ms, 3), device_ms_min=round(min(times[key]), 3), device_ms_max=round(max(times[key]), 3),
                       runs=args.runs, device_gbps=round(nbytes / ms / 1e6, 2), device_ratio=round(nbytes / written[key], 4),
                       frame_bytes=written[key], blocks=blocks[key])
            if args.tag:
                row["tag"] = args.tag
            if cpu and key == "flags 0":
                cms, cwritten, ver = cpu
                row.update(libzstd_version=ver, libzstd_level=1, libzstd_threads=args.threads, libzstd_ms=round(cms, 3),
                           libzstd_gbps=round(nbytes / cms / 1e6, 2), libzstd_ratio=round(nbytes / cwritten, 4))
            print(json.dumps(row), flush=True)
            rows.append(row)
        del d_in, d_out
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
