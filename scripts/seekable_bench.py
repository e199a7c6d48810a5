"""Device time of cz_seekable_pack_device (plan kernel included) and cz_seekable_open_device next to what a caller can do without
them, on two batches:
  records   the 100 000-record batch of scripts/compress_records_bench.py (records level, dictionaries, with the checksum)
  64x2MiB   64 buffers of 2 MiB tiled from the corpus, at CZ_COMPRESS_FAST_SPLIT with the checksum

Run it on the GPU box under a time limit of its own, e.g.
    timeout -k 10 500 python scripts/seekable_bench.py --out profiles/compress/seekable_bench.json
The frames lie in their slots of cz_compress_bound size in HBM, as the compress launch left them.  After one warm-up round the
ways alternate for --runs rounds; reported: the median, the fastest and the slowest of each.
  pack          events on the context's stream around cz_seekable_pack_device (both kernels)
  memcpy_each   (a) n hipMemcpyAsync device-to-device copies, one per frame, and a synchronise: host clock (the copies are issued
                from Python through ctypes, which is part of what is measured; the frame lengths are taken as known)
  host_concat   (b) the bounded region to pinned host memory, numpy concatenation of the frames, the stream back: host clock
  dtod_ceiling  one device-to-device copy of stream_bytes, events around it: what moving the bytes costs at least
  open          host clock around cz_seekable_open_device (all frames, out_align 256; it synchronises); open_events: events around
                the same call, the open kernel and the copy of the 56-byte info
  stream_split  cz_stream_split on a host copy of the same stream: host clock
The packed stream is compared with cz_seekable_pack_host's and the opened arrays with cz_seekable_open_host's.  The row `bar` says
whether, on the records batch, the slowest pack is faster than the fastest run of the faster of (a) and (b).  Prints one JSON line
per row and writes them to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def hip_runtime():
    """The HIP runtime this process already has mapped (torch's), through ctypes."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            h = C.CDLL(line.split()[-1])
            h.hipMemcpyAsync.restype = C.c_int
            h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            return h
    raise RuntimeError("no HIP runtime mapped")


def spread(t):
    t = sorted(t)
    return dict(runs=len(t), ms=round(float(np.median(t)), 4), ms_fastest=round(t[0], 4), ms_slowest=round(t[-1], 4))


def measure(name, cz, ctx, stream, hip, compress, n, lens, runs):
    """`compress(d_out, desc, d_res)` fills the slots; returns the rows of this batch."""
    import torch
    dev = torch.device("cuda:0")
    caps = np.array([cz.compress_bound(int(x)) for x in lens], dtype=np.uint64)
    out_off = np.zeros(n, dtype=np.uint64)
    out_off[1:] = np.cumsum(caps[:-1])
    region = int(caps.sum())
    d_out = torch.empty(region, dtype=torch.uint8, device=dev)
    d_off = torch.from_numpy(out_off.view(np.int64)).to(dev)
    d_cap = torch.from_numpy(caps.view(np.int64)).to(dev)
    d_res = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    cap = cz.seekable_bound(region, n, True)
    d_stream = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
    d_copy = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
    d_info = torch.zeros(56, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    compress(d_out, d_off, d_cap, d_res)
    ctx.synchronize()
    res = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)
    assert (res["status"] == 0).all()
    flen = res["bytes_written"].astype(np.int64)
    foff = out_off.astype(np.int64)
    dst = np.concatenate([[0], np.cumsum(flen[:-1])])
    h_pin = torch.empty(region, dtype=torch.uint8).pin_memory()
    h_stream_pin = torch.empty(cap, dtype=torch.uint8).pin_memory()

    def ev():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def pack():
        e0, e1 = ev()
        e0.record(stream)
        ctx.seekable_pack_device(d_out.data_ptr(), d_off.data_ptr(), d_res.data_ptr(), n, d_stream.data_ptr(), cap, d_info.data_ptr(), checksums=True)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def memcpy_each():
        src, to, sp = d_out.data_ptr(), d_copy.data_ptr(), stream.cuda_stream
        f = hip.hipMemcpyAsync
        t0 = time.perf_counter()
        for i in range(n):
            f(to + int(dst[i]), src + int(foff[i]), int(flen[i]), 3, sp)
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def host_concat():
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            h_pin.copy_(d_out, non_blocking=True)
        stream.synchronize()
        a = h_pin.numpy()
        packed = np.concatenate([a[o:o + k] for o, k in zip(foff, flen)])
        h_stream_pin[:packed.size] = torch.from_numpy(packed)
        with torch.cuda.stream(stream):
            d_copy[:packed.size].copy_(h_stream_pin[:packed.size], non_blocking=True)
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3

    pack()
    info = d_info.cpu().numpy().view(cz.SEEKABLE_INFO_DTYPE)[0]
    assert int(info["status"]) == 0
    sb, fb = int(info["stream_bytes"]), int(info["frames_bytes"])
    packed = d_stream.cpu().numpy()[:sb]
    # the same bytes as the host function's, from the slots as they came back
    h_out = d_out.cpu().numpy()
    h_stream, h_info = np.zeros(cap, dtype=np.uint8), np.zeros(1, dtype=cz.SEEKABLE_INFO_DTYPE)
    assert cz.lib().cz_seekable_pack_host(h_out.ctypes.data, out_off.ctypes.data, res.ctypes.data, n, h_stream.ctypes.data, cap, 1, h_info.ctypes.data) == 0
    assert h_info[0].tobytes() == info.tobytes() and (h_stream[:sb] == packed).all()

    def dtod():
        e0, e1 = ev()
        e0.record(stream)
        hip.hipMemcpyAsync(d_copy.data_ptr(), d_stream.data_ptr(), sb, 3, stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    arr = torch.zeros((4, n), dtype=torch.int64, device=dev)
    d_sum = torch.zeros(n, dtype=torch.int32, device=dev)

    def open_all():
        e0, e1 = ev()
        t0 = time.perf_counter()
        e0.record(stream)
        inf = ctx.seekable_open_device(d_stream.data_ptr(), sb, 0, None, 256, arr[0].data_ptr(), arr[1].data_ptr(), arr[2].data_ptr(),
                                       arr[3].data_ptr(), d_sum.data_ptr())
        wall = (time.perf_counter() - t0) * 1e3
        e1.record(stream)
        e1.synchronize()
        assert int(inf["status"]) == 0
        return wall, e0.elapsed_time(e1)

    host_copy = packed.copy()

    def split():
        t0 = time.perf_counter()
        st, ents, _ = cz.stream_split(host_copy)
        assert st == 0 and len(ents) == n + 1
        return (time.perf_counter() - t0) * 1e3

    ways = {"pack": pack, "memcpy_each": memcpy_each, "host_concat": host_concat, "dtod_ceiling": dtod, "stream_split": split}
    times = {k: [] for k in list(ways) + ["open", "open_events"]}
    for r in range(runs + 1):                                           # round 0 warms up
        for k, f in ways.items():
            ms = f()
            if r:
                times[k].append(ms)
            if k in ("memcpy_each", "host_concat") and r == 0:
                assert (d_copy.cpu().numpy()[:fb] == packed[:fb]).all(), k
        wall, kern = open_all()
        if r:
            times["open"].append(wall)
            times["open_events"].append(kern)
    want = cz.open_seekable(packed, 0, None, 256)
    got = arr.cpu().numpy().view(np.uint64)
    assert all((got[j] == want[1 + j]).all() for j in range(4)) and (d_sum.cpu().numpy().view(np.uint32) == want[5]).all()
    rows = []
    for k in times:
        row = dict(batch=name, way=k, frames=n, region_bytes=region, frames_bytes=fb, stream_bytes=sb, device=torch.cuda.get_device_name(0), **spread(times[k]))
        if k == "pack":
            ceil = float(np.median(times["dtod_ceiling"]))
            row.update(gbps_in_plus_out=round(2 * sb / row["ms"] / 1e6, 1), dtod_ceiling_over_pack=round(ceil / row["ms"], 3))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch
    import cairo_zstd_amd as cz
    import dict_records as dr
    from compress_bench import tiled
    hip = hip_runtime()
    stream = torch.cuda.Stream()
    ctx = cz.Context(0, stream.cuda_stream)
    dev = torch.device("cuda:0")

    def batch(bufs):
        lens = np.array([len(b) for b in bufs], dtype=np.uint64)
        in_off = np.zeros(len(bufs), dtype=np.uint64)
        in_off[1:] = np.cumsum(lens[:-1])
        d_in = torch.from_numpy(np.frombuffer(b"".join(bufs) + bytes(16), dtype=np.uint8).copy()).to(dev)
        d_desc = torch.from_numpy(np.stack([in_off, lens]).view(np.int64)).to(dev)
        return lens, d_in, d_desc

    rows = []
    recs = dr.records(args.records // 4, seed=1)
    bufs, idx = [b for _, b in recs], [j for j, _ in recs]
    dicts = [cz.Dictionary(ctx, d) for d in dr.dictionaries()]
    ctx.set_compress_dictionaries(dicts)
    lens, d_in, d_desc = batch(bufs)
    d_idx = torch.from_numpy(np.array(idx, dtype=np.uint32).view(np.int32)).to(dev)

    def records_level(d_out, d_off, d_cap, d_res):
        ctx.compress_batch_dict_device(d_in.data_ptr(), d_desc[0].data_ptr(), d_desc[1].data_ptr(), len(bufs), d_out.data_ptr(), d_off.data_ptr(),
                                       d_cap.data_ptr(), d_idx.data_ptr(), d_res.data_ptr(), checksum=True, records=True)

    rows += measure("records", cz, ctx, stream, hip, records_level, len(bufs), lens, args.runs)
    big = tiled(64, 2 << 20, seed=1)
    lens2, d_in2, d_desc2 = batch(big)

    def fast_split(d_out, d_off, d_cap, d_res):
        ctx.compress_batch_device(d_in2.data_ptr(), d_desc2[0].data_ptr(), d_desc2[1].data_ptr(), len(big), d_out.data_ptr(), d_off.data_ptr(),
                                  d_cap.data_ptr(), d_res.data_ptr(), checksum=True, fast_split=True)

    rows += measure("64x2MiB", cz, ctx, stream, hip, fast_split, len(big), lens2, args.runs)
    by = {(r["batch"], r["way"]): r for r in rows}
    p, a, b = by["records", "pack"], by["records", "memcpy_each"], by["records", "host_concat"]
    other = a if a["ms"] < b["ms"] else b
    rows.append(dict(batch="records", way="bar", pack_ms_slowest=p["ms_slowest"], faster_other=other["way"], other_ms_fastest=other["ms_fastest"],
                     pack_faster_beyond_the_spread=bool(p["ms_slowest"] < other["ms_fastest"]), speedup_median=round(other["ms"] / p["ms"], 1)))
    for r in rows:
        print(json.dumps(r), flush=True)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
