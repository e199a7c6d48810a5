"""Kernel time and frame bytes of the records level (CZ_COMPRESS_RECORDS) on many small records, next to the levels it stands beside:
with dictionaries the existing dictionary kernel (flags 0) and the records level; without dictionaries the plain compressor,
CZ_COMPRESS_FAST and the records level.

Run it on the GPU box under a time limit of its own, e.g.
    timeout -k 10 500 python scripts/compress_records_bench.py --out profiles/compress/records_bench.json
The batch is that of scripts/compress_dict_bench.py: --records records (110-420 bytes) of the four families of tests/dict_records.py,
interleaved, each with its family's dictionary.  Buffers lie in HBM; the figure is the kernel time from events around the launch.
After one warm-up round the configurations alternate for --runs rounds; reported: the median, the fastest and the slowest of each.
The first 64 records-level frames with dictionaries are read back by libzstd where the host has it.  Prints one JSON line per
configuration and writes them to --out."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dict_records as dr  # noqa: E402

CONFIGS = (("dict_kernel", True, {}), ("records_dict", True, {"records": True}),
           ("plain", False, {}), ("fast", False, {"fast": True}), ("records_plain", False, {"records": True}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=5)
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
    dev = torch.device("cuda:0")
    lens = np.array([len(b) for b in bufs], dtype=np.uint64)
    in_off = np.zeros(len(bufs), dtype=np.uint64)
    in_off[1:] = np.cumsum(lens[:-1])
    caps = np.array([cz.compress_bound(int(n)) for n in lens], dtype=np.uint64)
    out_off = np.zeros(len(bufs), dtype=np.uint64)
    out_off[1:] = np.cumsum(caps[:-1])
    d_in = torch.from_numpy(np.frombuffer(b"".join(bufs), dtype=np.uint8).copy()).to(dev)
    d_out = torch.empty(int(caps.sum()), dtype=torch.uint8, device=dev)
    desc = torch.from_numpy(np.stack([in_off, lens, out_off, caps]).view(np.int64)).to(dev)
    d_idx = torch.from_numpy(np.array(idx, dtype=np.uint32).view(np.int32)).to(dev)
    d_res = torch.zeros(len(bufs) * 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def launch(with_dict, kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        if with_dict:
            ctx.compress_batch_dict_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(bufs), d_out.data_ptr(),
                                           desc[2].data_ptr(), desc[3].data_ptr(), d_idx.data_ptr(), d_res.data_ptr(), **kw)
        else:
            ctx.compress_batch_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(bufs), d_out.data_ptr(),
                                      desc[2].data_ptr(), desc[3].data_ptr(), d_res.data_ptr(), **kw)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    times = {name: [] for name, _, _ in CONFIGS}
    written, readback = {}, None
    for r in range(args.runs + 1):                                      # round 0 warms up (and allocates each level's scratch)
        for name, with_dict, kw in CONFIGS:
            ms = launch(with_dict, kw)
            if r:
                times[name].append(ms)
            else:
                res = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)
                assert (res["status"] == 0).all(), name
                written[name] = int(res["bytes_written"].sum())
                if name == "records_dict" and dr.libzstd():
                    out = d_out.cpu().numpy()
                    for i in range(64):
                        f = out[int(out_off[i]):int(out_off[i]) + int(res[i]["bytes_written"])].tobytes()
                        assert dr.zstd_decompress_dict(f, len(bufs[i]), raw[idx[i]]) == bufs[i], i
                    readback = 64
    rows = []
    for name, with_dict, kw in CONFIGS:
        t = sorted(times[name])
        med = float(np.median(t))
        row = dict(batch=f"{len(bufs)} records", config=name, dictionaries=with_dict, input_bytes=nbytes, device=torch.cuda.get_device_name(0),
                   runs=len(t), kernel_ms=round(med, 3), kernel_ms_fastest=round(t[0], 3), kernel_ms_slowest=round(t[-1], 3),
                   gbps=round(nbytes / med / 1e6, 3), frame_bytes=written[name], ratio=round(nbytes / written[name], 4))
        if name == "records_dict":
            row["libzstd_read_back"] = readback
        print(json.dumps(row), flush=True)
        rows.append(row)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
