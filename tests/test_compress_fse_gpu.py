"""CZ_COMPRESS_FSE_TABLES on the MI355X (cz_compress_frames_fse_kernel, cz_compress_segments_fse_kernel): the flag is accepted where
it belongs and refused with dictionaries; frames with tables of their own decode under the oracle, libzstd and this library's decoder
(single launch and the pre-pass pipeline with checksums verified) and come out smaller than without the flag; host path = device
path; and the kernels without the flag write what they wrote before and after a launch with it.  Run with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import compress_frames as cf
import compress_fse as fx
from compress_split import blocks_of

pytestmark = pytest.mark.gpu
POISON, BLOCK = 0xEE, 128 << 10


@pytest.fixture(scope="module")
def cz():
    import torch  # noqa: F401
    import cairo_zstd_amd as m
    assert os.path.exists(m._lib.LIB_PATH), "libcairo_zstd_amd.so missing: run __graft_entry__.build()"
    return m


@pytest.fixture(scope="module")
def ctx(cz):
    c = cz.Context(0)
    yield c
    c.close()


def tiled(n, size, seed):
    """n buffers of `size` bytes cut from the concatenated corpus originals at shifting offsets."""
    pool = b"".join(b for _, b in cf.corpus_originals())
    pool = pool * (size // len(pool) + 2)
    rng = np.random.default_rng(seed)
    starts = rng.integers(0, len(pool) - size, n)
    return [pool[int(s):int(s) + size] for s in starts]


@pytest.fixture(scope="module")
def batch():
    return tiled(64, 128 << 10, seed=21)


def device_compress(cz, ctx, bufs, in_shift=3, checksum=False, split=False, fse_tables=True):
    """Through cz_compress_batch_device with torch buffers: inputs at odd offsets, output regions poisoned, the gaps between them
    checked.  Returns [(result, whole region)]."""
    import torch
    lens = [len(b) for b in bufs]
    in_off = np.cumsum([in_shift] + [n + 1 for n in lens[:-1]]).astype(np.uint64)
    host_in = np.zeros(int(in_off[-1]) + lens[-1] + 16, dtype=np.uint8)
    for o, b in zip(in_off, bufs):
        host_in[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    caps = [cz.compress_bound(n) for n in lens]
    out_off = np.cumsum([5] + [c + 3 for c in caps[:-1]]).astype(np.uint64)
    total = int(out_off[-1]) + caps[-1] + 64
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(host_in).to(dev)
    d_out = torch.full((total,), POISON, dtype=torch.uint8, device=dev)
    desc = torch.from_numpy(np.stack([in_off, np.array(lens, dtype=np.uint64), out_off, np.array(caps, dtype=np.uint64)]).view(np.int64)).to(dev)
    d_res = torch.zeros(len(bufs) * 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.compress_batch_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(bufs), d_out.data_ptr(), desc[2].data_ptr(),
                              desc[3].data_ptr(), d_res.data_ptr(), checksum=checksum, split=split, fse_tables=fse_tables)
    ctx.synchronize()
    out = d_out.cpu().numpy()
    res = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)
    assert (out[:int(out_off[0])] == POISON).all()
    ends = out_off + np.array(caps, dtype=np.uint64)
    for i in range(len(bufs) - 1):                                      # the 3-byte gaps between regions
        assert (out[int(ends[i]):int(out_off[i + 1])] == POISON).all(), i
    assert (out[int(ends[-1]):] == POISON).all()
    return [(res[i], out[int(out_off[i]):int(out_off[i]) + caps[i]].tobytes()) for i in range(len(bufs))]


def frames_of(cz, bufs, got, flags):
    """The frames of `got`, each checked: status, bound, poison past bytes_written, the record and its flags."""
    frames = []
    for i, (b, (r, region)) in enumerate(zip(bufs, got)):
        n = int(r["bytes_written"])
        assert int(r["status"]) == 0, (i, int(r["status"]))
        assert n <= cz.compress_bound(len(b))
        assert (np.frombuffer(region, dtype=np.uint8)[n:] == POISON).all(), f"frame {i}: bytes past bytes_written were touched"
        assert int(r["bytes_read"]) == len(b) and int(r["blocks"]) == max(1, -(-len(b) // BLOCK)), i
        assert int(r["flags"]) == flags, (i, int(r["flags"]))
        frames.append(region[:n])
    return frames


def decode_three_ways(cz, bufs, frames, checksum=False):
    """The oracle, libzstd where the host has it, then this library's decoder: the single launch and the pre-pass pipeline
    (cz_chain_kernel builds the tables there) with checksums verified."""
    import oracle
    for i, (b, fr) in enumerate(zip(bufs, frames)):
        st, out, info = oracle.decode_frame(fr, cap=len(b) + 64)
        assert st == 0 and out == b and info["consumed"] == len(fr) and info["content_size"] == len(b), i
        if cf.libzstd():
            assert cf.libzstd_decompress(fr, len(b)) == b, i
    for prepass in (False, True):
        dctx = cz.Context(0)
        if prepass:
            dctx.set_chain_arena(64 << 20, min_sequences=0)
            dctx.set_literal_arena(32 << 20)
            dctx.set_verify_checksum(True)
        dec = cz.decode_batch_host(frames, [len(b) + 64 for b in bufs], dctx)
        dctx.close()
        for i, (b, (r, out)) in enumerate(zip(bufs, dec)):
            assert int(r["status"]) == 0 and out == b, (i, prepass)
            if checksum and prepass:
                assert r["flags"] & cz.RESULT_CHECKSUM_MATCH, i


def test_flag_is_accepted_and_dictionaries_refuse(cz, ctx):
    """16 alone and with CHECKSUM and SPLIT in cz_compress_batch_device / _host; CZ_E_INVALID_ARG in cz_compress_batch_dict_*."""
    import torch
    assert cz.COMPRESS_FSE_TABLES == 16
    L = cz.lib()
    src = b"abcdabcdabcdabcd-abcdabcdabcdabcd" * 3
    cap = cz.compress_bound(len(src))
    d_in = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).to("cuda:0")
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    desc = torch.tensor([0, len(src), 0, cap], dtype=torch.int64, device="cuda:0")
    d_res = torch.zeros(32, dtype=torch.uint8, device="cuda:0")
    h_in, h_out = np.frombuffer(src, dtype=np.uint8).copy(), np.zeros(cap, dtype=np.uint8)
    h_desc, h_res = np.array([0, len(src), 0, cap], dtype=np.uint64), np.zeros(1, dtype=cz.COMPRESS_RESULT_DTYPE)
    for flags in (16, 16 | 1, 16 | 4, 16 | 4 | 1):
        st = L.cz_compress_batch_device(ctx._h, d_in.data_ptr(), desc[0:].data_ptr(), desc[1:].data_ptr(), 1, d_out.data_ptr(),
                                        desc[2:].data_ptr(), desc[3:].data_ptr(), flags, d_res.data_ptr())
        assert st == cz.status.CZ_OK, flags
        ctx.synchronize()
        r = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)[0]
        assert int(r["status"]) == 0 and int(r["flags"]) == flags & ~4     # (one segment: not split)
        dev = d_out.cpu().numpy()[:int(r["bytes_written"])].tobytes()
        st = L.cz_compress_batch_host(ctx._h, h_in.ctypes.data, h_in.size, h_desc[0:].ctypes.data, h_desc[1:].ctypes.data, 1,
                                      h_out.ctypes.data, h_out.size, h_desc[2:].ctypes.data, h_desc[3:].ctypes.data, flags, h_res.ctypes.data)
        assert st == cz.status.CZ_OK, flags
        assert int(h_res[0]["status"]) == 0 and int(h_res[0]["flags"]) == flags & ~4
        assert h_out[:int(h_res[0]["bytes_written"])].tobytes() == dev
        assert cf.libzstd() is None or cf.libzstd_decompress(dev, len(src)) == src
    p, hp = d_res.data_ptr(), h_res.ctypes.data
    for flags in (16, 16 | 1):
        assert L.cz_compress_batch_dict_device(ctx._h, p, p, p, 1, p, p, p, flags, p, p) == cz.status.CZ_E_INVALID_ARG
        assert L.cz_compress_batch_dict_host(ctx._h, hp, 8, hp, hp, 1, hp, 32, hp, hp, flags, hp, hp) == cz.status.CZ_E_INVALID_ARG


def test_corpus_three_decoders_and_size(cz, ctx):
    names, bufs = zip(*cf.corpus_originals())
    assert len(bufs) == 69
    got = cz.compress_batch_host(list(bufs), ctx, fse_tables=True)
    frames = [fr for _, fr in got]
    for name, b, (r, fr) in zip(names, bufs, got):
        assert int(r["status"]) == 0 and int(r["bytes_read"]) == len(b) and int(r["flags"]) == cz.COMPRESS_FSE_TABLES, name
        assert len(fr) <= cz.compress_bound(len(b))
    decode_three_ways(cz, bufs, frames)
    off = sum(len(fr) for _, fr in cz.compress_batch_host(list(bufs), ctx))
    total = sum(map(len, frames))
    used = [m for fr in frames for blk in fx.modes(fr) for m in (blk["ll"], blk["of"], blk["ml"])]
    print(f"corpus: {sum(map(len, bufs))} -> {total} bytes with the flag, {off} without; modes Predefined / RLE / FSE: "
          f"{used.count(0)} / {used.count(1)} / {used.count(2)}")
    assert total < off
    assert used.count(fx.FSE) > 0
    with_sum = cz.compress_batch_host(list(bufs[::3]), ctx, checksum=True, fse_tables=True)
    assert all(int(r["flags"]) == 17 for r, _ in with_sum)
    decode_three_ways(cz, bufs[::3], [fr for _, fr in with_sum], checksum=True)


def test_tiled_batch_keeps_poison_and_is_smaller(cz, ctx, batch):
    on = frames_of(cz, batch, device_compress(cz, ctx, batch), cz.COMPRESS_FSE_TABLES)
    off = frames_of(cz, batch, device_compress(cz, ctx, batch, fse_tables=False), 0)
    decode_three_ways(cz, batch, on)
    a, b = sum(map(len, on)), sum(map(len, off))
    print(f"64 x 128 KiB: ratio {sum(map(len, batch)) / a:.3f} with the flag, {sum(map(len, batch)) / b:.3f} without")
    assert a < b
    rev = frames_of(cz, batch[::-1], device_compress(cz, ctx, batch[::-1], in_shift=1), cz.COMPRESS_FSE_TABLES)[::-1]
    assert rev == on                                                    # the bytes do not depend on the batch


def test_split_with_the_flag(cz, ctx):
    S = cz.compress_split_segment()
    big = tiled(1, 3 << 20, seed=3)[0]
    (fs,) = frames_of(cz, [big], device_compress(cz, ctx, [big], split=True), cz.COMPRESS_FSE_TABLES | cz.COMPRESS_SPLIT)
    (fp,) = frames_of(cz, [big], device_compress(cz, ctx, [big]), cz.COMPRESS_FSE_TABLES)
    (hs, bs), (hp, bp) = blocks_of(fs), blocks_of(fp)
    assert hs == hp and len(bs) == len(bp) == 24 and [b[1] for b in bs] == [0] * 23 + [1]
    seg0 = bs[S // BLOCK][0]
    assert fs[:seg0] == fp[:seg0]
    assert any(m["ll"] == fx.FSE for m in fx.modes(fs)[S // BLOCK:])      # later segments have tables of their own too
    decode_three_ways(cz, [big], [fs])
    (plain,) = frames_of(cz, [big], device_compress(cz, ctx, [big], split=True, fse_tables=False), cz.COMPRESS_SPLIT)
    assert len(fs) < len(plain)
    small = big[:S]
    assert cz.compress(small, ctx, split=True, fse_tables=True) == cz.compress(small, ctx, fse_tables=True)


def test_host_path_matches_device_path(cz, ctx, batch):
    bufs = batch[:8] + [b"", b"a", b"\x00" * 300000, tiled(1, 700_000, seed=9)[0]]
    for split in (False, True):
        flags = cz.COMPRESS_FSE_TABLES
        got = device_compress(cz, ctx, bufs, split=split)
        dev = [region[:int(r["bytes_written"])] for r, region in got]
        assert all(int(r["status"]) == 0 and int(r["flags"]) & ~cz.COMPRESS_SPLIT == flags for r, _ in got)
        host = cz.compress_batch_host(bufs, ctx, split=split, fse_tables=True)
        assert [fr for _, fr in host] == dev
        assert [int(r["flags"]) for r, _ in host] == [int(r["flags"]) for r, _ in got]
    assert cz.compress(bufs[0], ctx, fse_tables=True) == dev[0]


def test_flag_off_is_unchanged_around_a_flag_on_launch(cz, ctx, batch):
    """No state leaks between the kernels: the frames without the flag before and after a launch with it are the same, and so are
    the frames with it."""
    before = [fr for _, fr in cz.compress_batch_host(batch, ctx, fse_tables=False)]
    on = [fr for _, fr in cz.compress_batch_host(batch, ctx, fse_tables=True)]
    after = [fr for _, fr in cz.compress_batch_host(batch, ctx, fse_tables=False)]
    again = [fr for _, fr in cz.compress_batch_host(batch, ctx, fse_tables=True)]
    assert before == after and on == again and on != before
    assert before == frames_of(cz, batch, device_compress(cz, ctx, batch, fse_tables=False), 0)
    assert all(m["ll"] == m["of"] == m["ml"] == fx.PREDEFINED for fr in before[:4] for m in fx.modes(fr))
