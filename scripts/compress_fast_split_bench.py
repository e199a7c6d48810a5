"""Speed of CZ_COMPRESS_FAST_SPLIT next to the two existing levels that it stands between, CZ_COMPRESS_FAST and
CZ_COMPRESS_SPLIT, measured in the same session on the same device.

Run it on the GPU box under a time limit of its own, e.g.
    timeout -k 10 600 python scripts/compress_fast_split_bench.py
Batches, tiled from the golden corpus originals as in scripts/compress_bench.py: 64 x 2 MiB (few, large buffers: the case the level
is for), 1 x 16 MiB (one buffer) and 10 000 x 128 KiB (every frame is ONE unit: what the plan launch and the search per unit cost
where there is nothing to gain).  Per batch the configurations alternate (fast, split, fast_split, fast_split + checksum, fast, ...)
for --runs rounds after one warm-up round; a row holds the median kernel time (hipEvents around the launch, plan kernel included,
inputs already in HBM), the fastest and slowest run, input bytes over the median, and the ratio.  The first 64 frames of every batch
and configuration are read back by libzstd where the host has it, and the fast_split frames must equal the fast frames byte for
byte.  The row `bar` says whether, on 64 x 2 MiB, the slowest fast_split run is faster than the fastest run of the faster existing
level: a margin beyond the run-to-run spread of the two.  The row `checksum_cost` holds what the one-wave XXH64 costs the checksum
variant on every batch.  Prints one JSON line per row and writes them all to --out (default profiles/compress/fast_split_bench.json)."""
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
from compress_bench import tiled  # noqa: E402

CONFIGS = (("fast", 32, dict(fast=True)), ("split", 4, dict(split=True)), ("fast_split", 128, dict(fast_split=True)),
           ("fast_split+checksum", 129, dict(fast_split=True, checksum=True)))
BATCHES = (("64x2MiB", 64, 2 << 20), ("1x16MiB", 1, 16 << 20), ("10000x128KiB", 10000, 128 << 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compress", "fast_split_bench.json"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tag", default=None, help="free text copied into every row")
    args = ap.parse_args()
    import torch
    import cairo_zstd_amd as cz
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()                                        # the context launches on it, the events are recorded on it
    ctx = cz.Context(0, stream.cuda_stream)
    rows = []
    for name, n, size in BATCHES:
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
        written, blocks, first = {}, {}, {}
        for r in range(args.runs + 1):
            for key, flags, kw in CONFIGS:
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
                k = min(n, 64)                                          # the frames are real: libzstd reads them back
                out = d_out[:k * int(caps[0])].cpu().numpy()
                first[key] = [out[int(out_off[i]):int(out_off[i]) + int(res[i]["bytes_written"])].tobytes() for i in range(k)]
                if cf.libzstd():
                    for i in range(k):
                        assert cf.libzstd_decompress(first[key][i], size) == bufs[i], (key, i)
        assert first["fast_split"] == first["fast"], "the fast_split frames are not the fast frames"
        for key, flags, _ in CONFIGS:
            ms = float(np.median(times[key]))
            row = dict(batch=name, config=key, flags=flags, input_bytes=nbytes, device=torch.cuda.get_device_name(0),
                       device_ms=round(ms, 3), device_ms_min=round(min(times[key]), 3), device_ms_max=round(max(times[key]), 3),
                       runs=args.runs, device_gbps=round(nbytes / ms / 1e6, 2), device_ratio=round(nbytes / written[key], 4),
                       frame_bytes=written[key], blocks=blocks[key])
            if args.tag:
                row["tag"] = args.tag
            print(json.dumps(row), flush=True)
            rows.append(row)
        med = {key: float(np.median(times[key])) for key, _, _ in CONFIGS}
        cost = dict(batch=name, row="checksum_cost", fast_split_ms=round(med["fast_split"], 3),
                    fast_split_checksum_ms=round(med["fast_split+checksum"], 3),
                    extra_ms=round(med["fast_split+checksum"] - med["fast_split"], 3))
        print(json.dumps(cost), flush=True)
        rows.append(cost)
        if name == "64x2MiB":
            best = min(("fast", "split"), key=lambda k: med[k])
            bar = dict(batch=name, row="bar", best_existing=best, best_existing_ms=round(med[best], 3),
                       best_existing_ms_min=round(min(times[best]), 3), fast_split_ms=round(med["fast_split"], 3),
                       fast_split_ms_max=round(max(times["fast_split"]), 3), speedup=round(med[best] / med["fast_split"], 2),
                       met=bool(max(times["fast_split"]) < min(times[best])))
            print(json.dumps(bar), flush=True)
            rows.append(bar)
        del d_in, d_out
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
