"""Seekable streams on the MI355X (cz_seekable_pack_device: cz_seekable_plan_kernel + cz_seekable_gather_kernel;
cz_seekable_open_device: cz_seekable_open_kernel).  The emulator's pack and open cases through the C ABI and through Python against
the model of the format (seekable_model.py) and the host functions, with poison intact in front of the stream, past stream_bytes
and everywhere on an error; the argument refusals; and the whole chain compress -> pack -> open -> decode on one context with no
host synchronisation between compress and pack, for records, for a range, and for large fast-split frames.  Run with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import dict_records as dr
import seekable_model as model
from test_emu_seekable import REFUSED, check_good, check_open, check_refused, open_cases, pack_cases

pytestmark = pytest.mark.gpu
ALL = 0xFFFFFFFFFFFFFFFF


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


def slots(frames):
    """The frames in one host buffer at odd offsets with gaps of 0x5A between them: (buffer, offsets)."""
    off, pos = [], 3
    for i, f in enumerate(frames):
        off.append(pos)
        pos += len(f) + 1 + i % 5
    buf = np.full(pos + 16, 0x5A, dtype=np.uint8)
    for o, f in zip(off, frames):
        buf[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return buf, np.array(off, dtype=np.uint64)


def device_pack(cz, ctx, c, via):
    """One PackCase through cz_seekable_pack_device (via "c": the C ABI, "py": Context.seekable_pack_device): (info, the whole block —
    residue bytes, the stream's cap, 64 more — 0xEE where nothing was written) and the same from cz_seekable_pack_host."""
    import torch
    dev = torch.device("cuda:0")
    buf, off = slots(c.frames)
    n = len(c.frames)
    d_buf = torch.from_numpy(buf).to(dev)
    d_off = torch.from_numpy(np.concatenate([off, np.zeros(1, dtype=np.uint64)]).view(np.int64)).to(dev)
    d_rec = torch.from_numpy(np.frombuffer(c.recs.tobytes() + bytes(32), dtype=np.uint8).copy()).to(dev)
    d_blk = torch.full((c.residue + c.cap + 64,), 0xEE, dtype=torch.uint8, device=dev)
    d_info = torch.full((56,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    if via == "c":
        st = cz.lib().cz_seekable_pack_device(ctx._h, d_buf.data_ptr(), d_off.data_ptr(), d_rec.data_ptr(), n, d_blk.data_ptr() + c.residue,
                                              c.cap, c.flags, d_info.data_ptr())
        assert st == 0
    else:
        ctx.seekable_pack_device(d_buf.data_ptr(), d_off.data_ptr(), d_rec.data_ptr(), n, d_blk.data_ptr() + c.residue, c.cap,
                                 d_info.data_ptr(), checksums=bool(c.flags))
    ctx.synchronize()
    info = d_info.cpu().numpy().view(cz.SEEKABLE_INFO_DTYPE)[0]
    h_blk = np.full(c.residue + c.cap + 64, 0xEE, dtype=np.uint8)
    h_info = np.zeros(1, dtype=cz.SEEKABLE_INFO_DTYPE)
    recs = np.frombuffer(c.recs.tobytes() + bytes(32), dtype=np.uint8).copy()
    st = cz.lib().cz_seekable_pack_host(buf.ctypes.data, off.ctypes.data if n else None, recs.ctypes.data, n, h_blk.ctypes.data + c.residue, c.cap,
                                        c.flags, h_info.ctypes.data)
    assert st == int(h_info[0]["status"])
    return info, d_blk.cpu().numpy().tobytes(), h_info[0], h_blk.tobytes()


@pytest.mark.parametrize("via", ("c", "py"))
def test_the_emulators_pack_cases(cz, ctx, via):
    """(Fails without the feature: the entry points do not exist.)"""
    for name, c in pack_cases().items():
        info, block, h_info, h_block = device_pack(cz, ctx, c, via)
        assert info.tobytes() == h_info.tobytes(), name
        assert block == h_block, f"{name}: the kernels' stream differs from cz_seekable_pack_host's"
        if name in REFUSED:
            check_refused(name, c, info, block)
        else:
            check_good(name, c, info, block)


@pytest.mark.parametrize("via", ("c", "py"))
def test_the_emulators_open_cases(cz, ctx, via):
    import torch
    dev = torch.device("cuda:0")
    L = cz.lib()
    for i, c in enumerate(open_cases()):
        k = c.k
        d_stream = torch.full((c.residue + len(c.stream) + 64,), 0x5A, dtype=torch.uint8, device=dev)
        if c.stream:
            d_stream[c.residue:c.residue + len(c.stream)] = torch.from_numpy(np.frombuffer(c.stream, dtype=np.uint8).copy())
        d_arr = torch.full((5, 8 * (k + 4)), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ptr = [d_arr[j].data_ptr() if c.arrays else 0 for j in range(5)]
        if via == "c":
            h_info = np.zeros(1, dtype=cz.SEEKABLE_INFO_DTYPE)
            st = L.cz_seekable_open_device(ctx._h, d_stream.data_ptr() + c.residue, len(c.stream), c.first, c.count, c.align,
                                           *[p or None for p in ptr], h_info.ctypes.data)
            info = h_info[0]
            assert st == int(info["status"]), i
        else:
            info = ctx.seekable_open_device(d_stream.data_ptr() + c.residue, len(c.stream), c.first, None if c.count == ALL else c.count, c.align, *ptr)
        raw = d_arr.cpu().numpy()
        arrays = [raw[j][:8 * k].view("<u8") for j in range(4)] + [raw[4][:4 * k].view("<u4")]
        check_open(i, c, info, arrays)
        assert (raw[:4, 8 * k:] == 0xA5).all() and (raw[4, 4 * k:] == 0xA5).all(), f"case {i}: an array was written past its range"
        h = cz.open_seekable(c.stream, c.first, None if c.count == ALL else c.count, c.align)
        assert info.tobytes() == h[0].tobytes(), i
        if int(info["status"]) == 0 and c.arrays:
            assert all(a.tolist() == b.tolist() for a, b in zip(arrays, h[1:])), i


def test_bit_and_argument_refusals(cz, ctx):
    """Unknown flag bits and n above the maximum in pack; out_align values that are not a power of two from 1 to 4096 and ranges
    outside the table in open: CZ_E_INVALID_ARG, nothing launched or nothing written."""
    import torch
    dev = torch.device("cuda:0")
    L = cz.lib()
    INVALID = cz.status.CZ_E_INVALID_ARG
    d = torch.full((256,), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = d.data_ptr()
    for flags in (2, 3, 4, 8, 0x80, 0x80000001):
        assert L.cz_seekable_pack_device(ctx._h, p, p, p, 0, p, 17, flags, p + 64) == INVALID, flags
    assert L.cz_seekable_pack_device(ctx._h, p, p, p, 0x8000001, p, 17, 0, p + 64) == INVALID
    assert L.cz_seekable_pack_device(ctx._h, p, p, p, 0, None, 17, 0, p + 64) == INVALID
    assert L.cz_seekable_pack_device(ctx._h, p, p, p, 0, p, 17, 0, None) == INVALID
    assert L.cz_seekable_pack_device(ctx._h, None, p, p, 1, p, 64, 0, p + 64) == INVALID
    ctx.synchronize()
    assert (d.cpu().numpy() == 0xEE).all()
    assert L.cz_seekable_pack_device(ctx._h, None, None, None, 0, p, 17, 0, p + 64) == 0          # n = 0 needs no source
    ctx.synchronize()
    assert d.cpu().numpy()[:17].tobytes() == model.build([], [])
    stream = model.build([b"abc", b"defgh"], [10, 20])
    d_stream = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).to(dev)
    d_arr = torch.full((5, 64), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ptr = [d_arr[j].data_ptr() for j in range(5)]
    for align in (0, 3, 6, 24, 4097, 8192, 0x80000000):
        info = ctx.seekable_open_device(d_stream.data_ptr(), len(stream), 0, None, align, *ptr)
        assert int(info["status"]) == INVALID and int(info["frames"]) == 0, align
    for first, count in ((3, 0), (3, None), (0, 3), (2, 1), (1, 2), (1, ALL - 1), (ALL, None)):
        info = ctx.seekable_open_device(d_stream.data_ptr(), len(stream), first, count, 1, *ptr)
        assert int(info["status"]) == INVALID and int(info["frames"]) == 2 and int(info["detail"]) == 0, (first, count)
    assert (d_arr.cpu().numpy() == 0xA5).all()
    for align in (1, 2, 4096):
        assert int(ctx.seekable_open_device(d_stream.data_ptr(), len(stream), 0, None, align, *ptr)["status"]) == 0


def compress_and_pack(cz, ctx, bufs, **kw):
    """bufs compressed with the checksum and packed with checksums, the pack enqueued directly behind the compress launch on the same
    context: (result records, pack info, packed stream)."""
    import torch
    dev = torch.device("cuda:0")
    n = len(bufs)
    lens = np.array([len(b) for b in bufs], dtype=np.uint64)
    in_off = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    caps = np.array([cz.compress_bound(int(x)) for x in lens], dtype=np.uint64)
    out_off = np.concatenate([[0], np.cumsum(caps[:-1] + np.uint64(3))]).astype(np.uint64)
    d_in = torch.from_numpy(np.frombuffer(b"".join(bufs) + bytes(16), dtype=np.uint8).copy()).to(dev)
    d_out = torch.full((int(out_off[-1] + caps[-1]) + 16,), 0xEE, dtype=torch.uint8, device=dev)
    desc = torch.from_numpy(np.stack([in_off, lens, out_off, caps]).view(np.int64)).to(dev)
    d_res = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    cap = cz.seekable_bound(int(caps.sum()), n, True)
    d_stream = torch.full((cap + 64,), 0xEE, dtype=torch.uint8, device=dev)
    d_info = torch.zeros(56, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.compress_batch_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), n, d_out.data_ptr(), desc[2].data_ptr(),
                              desc[3].data_ptr(), d_res.data_ptr(), checksum=True, **kw)
    ctx.seekable_pack_device(d_out.data_ptr(), desc[2].data_ptr(), d_res.data_ptr(), n, d_stream.data_ptr(), cap, d_info.data_ptr(), checksums=True)
    ctx.synchronize()
    res = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)
    info = d_info.cpu().numpy().view(cz.SEEKABLE_INFO_DTYPE)[0]
    assert int(info["status"]) == 0 and (res["status"] == 0).all()
    whole = d_stream.cpu().numpy()
    sb = int(info["stream_bytes"])
    assert (whole[sb:] == 0xEE).all()
    out = d_out.cpu().numpy()
    frames = [out[int(o):int(o) + int(r["bytes_written"])].tobytes() for o, r in zip(out_off, res)]
    assert whole[:sb].tobytes() == model.build(frames, [len(b) for b in bufs], [int(r["checksum"]) for r in res])
    return res, info, whole[:sb].tobytes()


def open_and_decode(cz, dctx, packed, first, count):
    """The sizing call, then the arrays at out_align 1, then one decode_batch_device on them with checksums verified:
    (decoded bytes per frame, result records, the table's checksums, out_off, out_cap)."""
    import torch
    dev = torch.device("cuda:0")
    d_stream = torch.from_numpy(np.frombuffer(packed + bytes(64), dtype=np.uint8).copy()).to(dev)
    torch.cuda.synchronize()
    size = dctx.seekable_open_device(d_stream.data_ptr(), len(packed), first, count, 1)
    assert int(size["status"]) == 0
    k = int(size["frames"]) - first if count is None else count
    desc = torch.zeros((4, k), dtype=torch.int64, device=dev)
    d_sum = torch.zeros(k, dtype=torch.int32, device=dev)
    d_out = torch.full((int(size["detail"]) + 64,), 0xEE, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(k * cz.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    info = dctx.seekable_open_device(d_stream.data_ptr(), len(packed), first, count, 1, desc[0].data_ptr(), desc[1].data_ptr(), desc[2].data_ptr(),
                                     desc[3].data_ptr(), d_sum.data_ptr())
    assert info.tobytes() == size.tobytes()
    dctx.decode_batch_device(d_stream.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), k, d_out.data_ptr(), desc[2].data_ptr(), desc[3].data_ptr(),
                             d_res.data_ptr())
    dctx.synchronize()
    res = d_res.cpu().numpy().view(cz.RESULT_DTYPE)
    out, h = d_out.cpu().numpy(), desc.cpu().numpy().view(np.uint64)
    assert (out[int(size["detail"]):] == 0xEE).all()
    return [out[int(o):int(o) + int(c)].tobytes() for o, c in zip(h[2], h[3])], res, d_sum.cpu().numpy().view(np.uint32), h[2], h[3]


@pytest.fixture(scope="module")
def records_chain(cz, ctx):
    bufs = [b for _, b in dr.records(1000, seed=11)]
    assert len(bufs) == 4000
    res, info, packed = compress_and_pack(cz, ctx, bufs, records=True)
    dctx = cz.Context(0)
    dctx.set_verify_checksum(True)
    yield bufs, res, info, packed, dctx
    dctx.close()


def check_decoded(cz, bufs, res, got):
    """Outputs equal inputs; calculated_checksum equals the table's value (and the compressor's) for every frame; with out_align 1
    the caps are exact and the outputs lie back to back."""
    outs, dres, sums, out_off, out_cap = got
    assert outs == bufs
    assert (dres["status"] == 0).all() and (dres["flags"] & cz.RESULT_CHECKSUM_MATCH).all()
    assert dres["calculated_checksum"].tolist() == sums.tolist() == [int(r["checksum"]) for r in res]
    assert out_cap.tolist() == [len(b) for b in bufs] == dres["bytes_produced"].tolist()
    assert out_off.tolist() == np.concatenate([[0], np.cumsum(out_cap[:-1])]).tolist()


def test_records_compress_pack_open_decode(cz, records_chain):
    bufs, res, info, packed, dctx = records_chain
    assert int(info["frames"]) == 4000 and int(info["content_bytes"]) == sum(map(len, bufs)) and int(info["has_checksums"]) == 1
    assert (res["flags"] == (cz.COMPRESS_RECORDS | cz.COMPRESS_CHECKSUM)).all()
    check_decoded(cz, bufs, res, open_and_decode(cz, dctx, packed, 0, None))


def test_records_a_range_of_ten(cz, records_chain):
    bufs, res, info, packed, dctx = records_chain
    check_decoded(cz, bufs[1000:1010], res[1000:1010], open_and_decode(cz, dctx, packed, 1000, 10))


def test_fast_split_frames_and_an_empty_input(cz, ctx):
    import compress_edges as ce
    text = ce.corpus_text(64 << 10)
    pool = text * 7
    bufs = [pool[101 * i + 1: 101 * i + 1 + (300 << 10)] for i in range(3)] + [b""]
    res, info, packed = compress_and_pack(cz, ctx, bufs, fast_split=True)
    assert int(info["frames"]) == 4 and (res["flags"] == (cz.COMPRESS_FAST_SPLIT | cz.COMPRESS_CHECKSUM)).all()
    dctx = cz.Context(0)
    dctx.set_verify_checksum(True)
    try:
        check_decoded(cz, bufs, res, open_and_decode(cz, dctx, packed, 0, None))
        check_decoded(cz, bufs[3:], res[3:], open_and_decode(cz, dctx, packed, 3, 1))
        assert cz.decode_stream(packed, dctx) == b"".join(bufs) == b"".join(cz.decode_seekable(packed, dctx))
    finally:
        dctx.close()


def test_decode_stream_and_decode_seekable_agree(cz, records_chain):
    bufs, res, info, packed, dctx = records_chain
    small = cz.pack_seekable(*zip(*[(packed[a:a + n], len(b)) for a, n, b in zip(*model.open_range(packed)[1:3], bufs)][:300]))
    assert cz.decode_stream(small, dctx) == b"".join(bufs[:300])
    assert cz.decode_seekable(small, dctx) == bufs[:300]
    assert cz.decode_seekable(packed, dctx, 3990) == bufs[3990:] and cz.decode_seekable(packed, dctx, 7, 2) == bufs[7:9]
    assert cz.decode_seekable(packed, dctx, 4000) == []
    with pytest.raises(cz.CzError):
        cz.decode_seekable(packed, dctx, 4001)
    with pytest.raises(cz.CzError):
        cz.decode_seekable(packed[:-1], dctx)


def test_other_levels_are_unchanged_around_a_pack_launch(cz, ctx):
    """Frames of flags 0, 32, 64 and 128 on the same context, before and after a pack: no state leaks between the kernels."""
    import compress_edges as ce
    text = ce.corpus_text(64 << 10)
    some = [(text * 6)[53 * i: 53 * i + (200 << 10)] for i in range(4)] + [text[:5000], b""]
    small = [b[:20000] for b in some]

    def others():
        return [[fr for _, fr in cz.compress_batch_host(some, ctx, **kw)] for kw in ({}, {"fast": True}, {"fast_split": True})] \
            + [[fr for _, fr in cz.compress_batch_host(small, ctx, records=True)]]

    before = others()
    _, _, packed = compress_and_pack(cz, ctx, some, fast_split=True)
    after = others()
    assert before == after
    assert len(packed) == cz.seekable_bound(sum(len(f) + 4 for f in before[2]), len(some), True)
