"""Reading byte ranges out of a seekable stream in HBM: index + locate + decode of the touched frames + gather
(cz_seekable_index_create_device, cz_seekable_locate_device, cz_decode_batch_device, cz_seekable_gather_device) next to what a caller
can do without them, on two streams:
  records   the 100 000-record stream of scripts/seekable_bench.py (records level, dictionaries, with the checksum)
            A1: 1 000 random whole records        A2: 1 000 random 64-byte slices
  64x2MiB   64 buffers of 2 MiB tiled from the corpus, at CZ_COMPRESS_FAST_SPLIT with the checksum
            B: 1 000 random 4 KiB slices

Run it on the GPU box under a time limit of its own, e.g.
    timeout -k 10 500 python scripts/seekable_read_bench.py --out profiles/compress/seekable_read_bench.json
One session; after one warm-up round the ways alternate for --runs rounds; reported: the median, the fastest and the slowest of each.
  new           locate (arrays and spans, frames_cap = all frames) + decode_batch_device of the k frames + gather, by the host clock up
                to a final synchronise; the index is built beforehand (index_build: host clock around the build, it synchronises)
  memcpy_each   (a) cz_seekable_open_device of all frames, decode_batch_device of all frames, m hipMemcpyAsync device-to-device copies
                (issued from Python through ctypes, which is part of what is measured; the source offsets are taken as known) and a
                synchronise: host clock
  torch_cat     (b) the same open and decode, the slices taken by ONE torch.cat of device views and a synchronise: host clock
  locate        the locate alone, host clock (it synchronises)
  decode_selected  decode_batch_device of the k frames alone, events around it
  gather        the gather alone, events around it
  dtod_ceiling  one device-to-device copy of dst_bytes, events around it: what moving the bytes costs at least
The gathered bytes are compared with cz_seekable_locate_host + cz_seekable_gather_host on the decoded frames, and with what (a) and
(b) give.  The row `bar` says whether, on A1, the slowest `new` is faster than the fastest run of the faster of (a) and (b).  Prints
one JSON line per row and writes them to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from seekable_bench import hip_runtime, spread  # noqa: E402


def packed_stream(cz, ctx, compress, n, lens):
    """`compress(d_out, d_off, d_cap, d_res)` fills the slots; the packed stream in HBM: (tensor, stream_bytes)."""
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
    d_info = torch.zeros(56, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    compress(d_out, d_off, d_cap, d_res)
    ctx.seekable_pack_device(d_out.data_ptr(), d_off.data_ptr(), d_res.data_ptr(), n, d_stream.data_ptr(), cap, d_info.data_ptr(), checksums=True)
    ctx.synchronize()
    info = d_info.cpu().numpy().view(cz.SEEKABLE_INFO_DTYPE)[0]
    assert int(info["status"]) == 0
    return d_stream, int(info["stream_bytes"])


def measure(name, read, cz, ctx, stream, hip, d_stream, sb, lens, ranges, runs):
    import torch
    dev = torch.device("cuda:0")
    n, m = len(lens), len(ranges)
    r = np.array(ranges, dtype=np.uint64).reshape(m, 2)
    d_rng = torch.from_numpy(np.ascontiguousarray(r.T).view(np.int64).copy()).to(dev)
    rp = (d_rng[0].data_ptr(), d_rng[1].data_ptr(), m)
    t_index = []
    ix = None
    for _ in range(runs + 1):
        if ix is not None:
            ix.close()
        t0 = time.perf_counter()
        ix = ctx.seekable_index(d_stream.data_ptr(), sb)
        t_index.append((time.perf_counter() - t0) * 1e3)
    size = ix.locate(*rp, 256)
    assert int(size["status"]) == 0
    k, dst_bytes, out_bytes = int(size["selected"]), int(size["dst_bytes"]), int(size["out_bytes"])
    opened = ctx.seekable_open_device(d_stream.data_ptr(), sb, 0, None, 256)
    full_bytes = int(opened["detail"])
    desc = torch.zeros((5, n), dtype=torch.int64, device=dev)           # in_off, in_len, out_off, out_cap, content_off
    d_u32 = torch.zeros((2, n), dtype=torch.int32, device=dev)          # frame, checksum
    d_spans = torch.zeros(m * 24, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(out_bytes + 256, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(n * cz.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_dst = torch.zeros(dst_bytes + 16, dtype=torch.uint8, device=dev)
    d_copy = torch.zeros(dst_bytes + 16, dtype=torch.uint8, device=dev)
    arr = torch.zeros((4, n), dtype=torch.int64, device=dev)
    d_full = torch.zeros(full_bytes + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def ev():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def locate():
        t0 = time.perf_counter()
        info = ix.locate(*rp, 256, n, d_u32[0].data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), desc[2].data_ptr(), desc[3].data_ptr(),
                         d_u32[1].data_ptr(), desc[4].data_ptr(), d_spans.data_ptr())
        assert int(info["status"]) == 0 and int(info["selected"]) == k
        return (time.perf_counter() - t0) * 1e3

    def gather_call():
        ctx.seekable_gather_device(d_out.data_ptr(), desc[2].data_ptr(), desc[4].data_ptr(), k, rp[0], rp[1], d_spans.data_ptr(), m,
                                   d_dst.data_ptr(), dst_bytes)

    def new():
        t0 = time.perf_counter()
        locate()
        ctx.decode_batch_device(d_stream.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), k, d_out.data_ptr(), desc[2].data_ptr(),
                                desc[3].data_ptr(), d_res.data_ptr())
        gather_call()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def decode_selected():
        e0, e1 = ev()
        e0.record(stream)
        ctx.decode_batch_device(d_stream.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), k, d_out.data_ptr(), desc[2].data_ptr(),
                                desc[3].data_ptr(), d_res.data_ptr())
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def gather():
        e0, e1 = ev()
        e0.record(stream)
        gather_call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    # where each range lies in a decode of ALL frames at out_align 256 (taken as known by the two other ways)
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    full_off = np.concatenate([[0], np.cumsum((np.asarray(lens, dtype=np.int64) + 255) // 256 * 256)])[:-1]
    pieces = []                                                          # (source offset in d_full, length) in destination order
    for o, ln in ranges:
        f = int(np.searchsorted(starts, o, side="right")) - 1
        while ln:
            while lens[f] == 0 or starts[f + 1] <= o:
                f += 1
            take = min(ln, int(starts[f + 1]) - o)
            pieces.append((int(full_off[f]) + o - int(starts[f]), take))
            o, ln = o + take, ln - take
    piece_dst = np.concatenate([[0], np.cumsum([p[1] for p in pieces])])

    def open_and_decode_all():
        inf = ctx.seekable_open_device(d_stream.data_ptr(), sb, 0, None, 256, arr[0].data_ptr(), arr[1].data_ptr(), arr[2].data_ptr(), arr[3].data_ptr())
        assert int(inf["status"]) == 0
        ctx.decode_batch_device(d_stream.data_ptr(), arr[0].data_ptr(), arr[1].data_ptr(), n, d_full.data_ptr(), arr[2].data_ptr(), arr[3].data_ptr(),
                                d_res.data_ptr())

    def memcpy_each():
        src, to, sp = d_full.data_ptr(), d_copy.data_ptr(), stream.cuda_stream
        f = hip.hipMemcpyAsync
        t0 = time.perf_counter()
        open_and_decode_all()
        for (s, ln), d in zip(pieces, piece_dst):
            f(to + int(d), src + s, ln, 3, sp)
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3

    cat_out = [None]

    def torch_cat():
        t0 = time.perf_counter()
        open_and_decode_all()
        with torch.cuda.stream(stream):
            cat_out[0] = torch.cat([d_full[s:s + ln] for s, ln in pieces]) if pieces else d_full[:0]
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def dtod():
        e0, e1 = ev()
        e0.record(stream)
        hip.hipMemcpyAsync(d_copy.data_ptr(), d_dst.data_ptr(), dst_bytes, 3, stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    ways = {"new": new, "memcpy_each": memcpy_each, "torch_cat": torch_cat, "locate": locate, "decode_selected": decode_selected, "gather": gather, "dtod_ceiling": dtod}
    times = {w: [] for w in ways}
    want = None
    for rnd in range(runs + 1):                                         # round 0 warms up
        for w, f in ways.items():
            ms = f()
            if rnd:
                times[w].append(ms)
            if rnd == 0 and w == "new":
                # the same bytes as the host functions give on the frames as they were decoded
                res = d_res.cpu().numpy().view(cz.RESULT_DTYPE)[:k]
                assert (res["status"] == 0).all()
                packed = d_stream.cpu().numpy()[:sb]
                hinfo, _, _, _, hout_off, _, _, hcontent_off, hspans = cz.locate_seekable(packed, ranges, 256)
                assert int(hinfo["status"]) == 0 and int(hinfo["selected"]) == k
                assert (desc[2][:k].cpu().numpy().view(np.uint64) == hout_off).all() and (d_spans.cpu().numpy().view(cz.SEEKABLE_SPAN_DTYPE) == hspans).all()
                h_dec, h_dst = d_out.cpu().numpy(), np.zeros(dst_bytes + 1, dtype=np.uint8)
                off, ln = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
                assert cz.lib().cz_seekable_gather_host(h_dec.ctypes.data, hout_off.ctypes.data, hcontent_off.ctypes.data, k, off.ctypes.data, ln.ctypes.data,
                                                        hspans.ctypes.data, m, h_dst.ctypes.data, dst_bytes) == 0
                want = h_dst[:dst_bytes]
                assert (d_dst.cpu().numpy()[:dst_bytes] == want).all(), "gather differs from the host functions"
            if rnd == 0 and w == "memcpy_each":
                assert (d_copy.cpu().numpy()[:dst_bytes] == want).all(), w
            if rnd == 0 and w == "torch_cat":
                assert (cat_out[0].cpu().numpy() == want).all(), w
    ix.close()
    rows = [dict(stream=name, read=read, way="index_build", frames=n, **spread(t_index[1:]))]
    for w in times:
        row = dict(stream=name, read=read, way=w, frames=n, ranges=m, selected=k, dst_bytes=dst_bytes, decoded_bytes=out_bytes, stream_bytes=sb,
                   device=torch.cuda.get_device_name(0), **spread(times[w]))
        if w == "gather":
            row.update(gbps_in_plus_out=round(2 * dst_bytes / row["ms"] / 1e6, 2), dtod_ceiling_over_gather=round(float(np.median(times["dtod_ceiling"])) / row["ms"], 3))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--ranges", type=int, default=1000)
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
    rng = np.random.default_rng(1)

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
    ctx.set_dictionaries(dicts)
    lens, d_in, d_desc = batch(bufs)
    d_idx = torch.from_numpy(np.array(idx, dtype=np.uint32).view(np.int32)).to(dev)

    def records_level(d_out, d_off, d_cap, d_res):
        ctx.compress_batch_dict_device(d_in.data_ptr(), d_desc[0].data_ptr(), d_desc[1].data_ptr(), len(bufs), d_out.data_ptr(), d_off.data_ptr(),
                                       d_cap.data_ptr(), d_idx.data_ptr(), d_res.data_ptr(), checksum=True, records=True)

    d_stream, sb = packed_stream(cz, ctx, records_level, len(bufs), lens)
    ilens = lens.astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(ilens)])
    pick = rng.integers(0, len(bufs), args.ranges)
    a1 = [(int(starts[i]), int(ilens[i])) for i in pick]
    a2 = [(int(starts[i]) + int(rng.integers(0, max(int(ilens[i]) - 64, 1))), min(64, int(ilens[i]))) for i in rng.integers(0, len(bufs), args.ranges)]
    rows += measure("records", "A1", cz, ctx, stream, hip, d_stream, sb, ilens, a1, args.runs)
    rows += measure("records", "A2", cz, ctx, stream, hip, d_stream, sb, ilens, a2, args.runs)
    del d_stream
    big = tiled(64, 2 << 20, seed=1)
    lens2, d_in2, d_desc2 = batch(big)

    def fast_split(d_out, d_off, d_cap, d_res):
        ctx.compress_batch_device(d_in2.data_ptr(), d_desc2[0].data_ptr(), d_desc2[1].data_ptr(), len(big), d_out.data_ptr(), d_off.data_ptr(),
                                  d_cap.data_ptr(), d_res.data_ptr(), checksum=True, fast_split=True)

    d_stream2, sb2 = packed_stream(cz, ctx, fast_split, len(big), lens2)
    content = int(lens2.sum())
    b = [(int(o), 4096) for o in rng.integers(0, content - 4096, args.ranges)]
    rows += measure("64x2MiB", "B", cz, ctx, stream, hip, d_stream2, sb2, lens2.astype(np.int64), b, args.runs)
    by = {(r["read"], r["way"]): r for r in rows}
    p, a, c = by["A1", "new"], by["A1", "memcpy_each"], by["A1", "torch_cat"]
    other = a if a["ms"] < c["ms"] else c
    rows.append(dict(stream="records", read="A1", way="bar", new_ms_slowest=p["ms_slowest"], faster_other=other["way"], other_ms_fastest=other["ms_fastest"],
                     new_faster_beyond_the_spread=bool(p["ms_slowest"] < other["ms_fastest"]), speedup_median=round(other["ms"] / p["ms"], 1)))
    for r in rows:
        print(json.dumps(r), flush=True)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
