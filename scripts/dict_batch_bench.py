#!/usr/bin/env python3
"""Times batch decodes with dictionaries (cz_context_set_dictionary / cz_context_set_dictionaries) on the committed fixtures of
tests/golden/multidict, repeated to --frames frames.  Legs, run alternately --rounds times after a warm-up:

  a  one dictionary's frames, cz_context_set_dictionary(that dictionary)
  b  the same frames, cz_context_set_dictionaries(all four)
  c  the four dictionaries' frames mixed, one launch with cz_context_set_dictionaries(all four)
  d  the same mix as four launches, one per dictionary, each behind cz_context_set_dictionary (the way to decode such a batch
     without several dictionaries: split by dictionary, launch per group; the split itself is made once, outside the timing)

Kernel time is cz_context_last_kernel_ms (leg d: the sum over its four launches); wall time is the host's, from the first
settings call to the end of the last launch, synchronisations included.  Every frame of every run is checked against its
original (sha256).  Prints one JSON line per leg (and writes them to the file --out names, if any)."""
import argparse
import hashlib
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class Batch:
    """Device buffers of one batch (the same on every launch)."""

    def __init__(self, cz, frames):
        import torch
        dev = torch.device("cuda:0")
        self.cz, self.frames, self.n = cz, frames, len(frames)
        lens = np.array([len(f.zst) for f in frames], dtype=np.int64)
        self.caps = np.array([f.orig_len + 64 for f in frames], dtype=np.int64)
        pad = (self.caps + 255) // 256 * 256
        self.out_off = np.concatenate([[0], np.cumsum(pad)[:-1]]).astype(np.int64)
        self.t_in = torch.from_numpy(np.frombuffer(b"".join(f.zst for f in frames) + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        self.t_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)).to(dev)
        self.t_len = torch.from_numpy(lens).to(dev)
        self.t_ooff, self.t_ocap = torch.from_numpy(self.out_off).to(dev), torch.from_numpy(self.caps).to(dev)
        self.t_out = torch.empty(int(pad.sum()), dtype=torch.uint8, device=dev)
        self.t_res = torch.zeros(self.n * cz.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)

    def launch(self, ctx):
        ctx.decode_batch_device(self.t_in.data_ptr(), self.t_off.data_ptr(), self.t_len.data_ptr(), self.n, self.t_out.data_ptr(),
                                self.t_ooff.data_ptr(), self.t_ocap.data_ptr(), self.t_res.data_ptr())

    def check(self):
        res, out = self.t_res.cpu().numpy().view(self.cz.RESULT_DTYPE), self.t_out.cpu().numpy()
        bad = 0
        for i, f in enumerate(self.frames):
            lo = int(self.out_off[i])
            if int(res[i]["status"]) != 0 or int(res[i]["bytes_produced"]) != f.orig_len or \
                    hashlib.sha256(out[lo:lo + f.orig_len].tobytes()).hexdigest() != f.meta["orig_sha256"]:
                bad += 1
        return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    import torch
    import cairo_zstd_amd as cz
    import multidict_data as md
    ctx = cz.Context(0)
    ctx.set_chain_arena(1 << 30, min_sequences=0)
    ctx.set_literal_arena(1 << 30)
    dicts = {n: cz.Dictionary(ctx, md.dict_bytes(n)) for n in md.REGISTERED}
    per = {n: [f for f in md.registered_frames() if f.dictionary == n] for n in md.REGISTERED}
    one = Batch(cz, (per["dict_a"] * (args.frames // len(per["dict_a"]) + 1))[:args.frames])
    mix_frames = []
    for n in md.REGISTERED:
        mix_frames += (per[n] * (args.frames // (4 * len(per[n])) + 1))[:args.frames // 4]
    random.Random(11).shuffle(mix_frames)
    mix = Batch(cz, mix_frames)
    groups = {n: Batch(cz, [f for f in mix_frames if f.dictionary == n]) for n in md.REGISTERED}   # leg d: the split, made once

    def leg_a():
        ctx.set_dictionary(dicts["dict_a"]); one.launch(ctx); torch.cuda.synchronize()
        return ctx.last_kernel_ms(), [one]

    def leg_b():
        ctx.set_dictionaries(list(dicts.values())); one.launch(ctx); torch.cuda.synchronize()
        return ctx.last_kernel_ms(), [one]

    def leg_c():
        ctx.set_dictionaries(list(dicts.values())); mix.launch(ctx); torch.cuda.synchronize()
        return ctx.last_kernel_ms(), [mix]

    def leg_d():
        ms = 0.0
        for n in md.REGISTERED:
            ctx.set_dictionary(dicts[n]); groups[n].launch(ctx); torch.cuda.synchronize()
            ms += ctx.last_kernel_ms()
        return ms, list(groups.values())

    legs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d}
    kern = {k: [] for k in legs}
    wall = {k: [] for k in legs}
    bad = {k: 0 for k in legs}
    for r in range(args.warmup + args.rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ms, batches = fn()
            t1 = time.perf_counter()
            for b in batches:
                bad[k] += b.check()
            if r >= args.warmup:
                kern[k].append(ms); wall[k].append((t1 - t0) * 1e3)
    ctx.set_dictionary(None)
    lines = []
    for k in legs:
        ks, ws = np.array(kern[k]), np.array(wall[k])
        lines.append({"leg": k, "frames": args.frames, "rounds": args.rounds, "kernel_ms_median": round(float(np.median(ks)), 4),
                      "kernel_ms_min": round(float(ks.min()), 4), "kernel_ms_max": round(float(ks.max()), 4),
                      "wall_ms_median": round(float(np.median(ws)), 4), "wall_ms_min": round(float(ws.min()), 4),
                      "wall_ms_max": round(float(ws.max()), 4), "frames_wrong": bad[k]})
    for l in lines:
        print(json.dumps(l))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))
    for d in dicts.values():
        d.close()
    ctx.close()
    if any(bad.values()):
        sys.exit(f"frames decoded wrong: {bad}")


if __name__ == "__main__":
    main()
