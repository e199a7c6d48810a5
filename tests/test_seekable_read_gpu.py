"""Byte ranges out of a seekable stream on the MI355X (cz_seekable_index_create_device: cz_seekable_open_kernel +
cz_seekable_index_kernel; cz_seekable_locate_device: cz_seekable_locate_kernel + cz_seekable_select_kernel;
cz_seekable_gather_device: cz_seekable_ranges_kernel).  The emulator's locate and gather cases through the C ABI and through Python
against the model (seekable_read_model.py), with poison intact in the arrays on a refusal, in front of the destination and past
dst_bytes; the host-side argument refusals; and the whole chain compress -> pack -> index -> locate -> decode -> gather on one
context, for records, for large fast-split frames and through read_seekable.  Run with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import dict_records as dr
import seekable_model as fmt
import seekable_read_model as model
from test_emu_seekable_read import check_call, check_gathered, damaged_cases, gather_cases, locate_cases
from test_seekable_gpu import compress_and_pack

pytestmark = pytest.mark.gpu
SPAN = 24


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


def to_device(a):
    """A numpy array (any dtype) as a uint8 tensor on the device, never empty."""
    import torch
    raw = np.frombuffer(a.tobytes() + bytes(16), dtype=np.uint8).copy()
    return torch.from_numpy(raw).to("cuda:0")


def stage(stream, residue=1):
    """The stream in HBM `residue` bytes into a tensor: (tensor, pointer)."""
    import torch
    t = torch.full((residue + len(stream) + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
    t[residue:residue + len(stream)] = torch.from_numpy(np.frombuffer(bytes(stream), dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + residue


class Located:
    """One locate on the device: the info record and, when arrays were asked for, the seven arrays and the spans as device tensors
    of k_alloc and m entries (0xA5 where nothing was written)."""

    TYPES = (np.uint32, np.uint64, np.uint64, np.uint64, np.uint64, np.uint32, np.uint64)

    def __init__(self, cz, ix, ranges, align, frames_cap, k_alloc, arrays, via):
        import torch
        self.m = m = len(ranges)
        r = np.array(ranges, dtype=np.uint64).reshape(m, 2)
        self.d_off, self.d_len = to_device(np.ascontiguousarray(r[:, 0])), to_device(np.ascontiguousarray(r[:, 1]))
        self.k_alloc = k_alloc
        self.d_arr = [torch.full((k_alloc * np.dtype(t).itemsize + 16,), 0xA5, dtype=torch.uint8, device="cuda:0") for t in self.TYPES]
        self.d_spans = torch.full((m * SPAN + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ptr = [t.data_ptr() for t in self.d_arr] + [self.d_spans.data_ptr()] if arrays else [0] * 8
        rp = (self.d_off.data_ptr(), self.d_len.data_ptr()) if m else (0, 0)
        if via == "c":
            info = np.zeros(1, dtype=cz.SEEKABLE_READ_INFO_DTYPE)
            h = ix._h if isinstance(ix, cz.SeekableIndex) else ix
            self.ret = cz.lib().cz_seekable_locate_device(h, rp[0] or None, rp[1] or None, m, align, frames_cap, *[p or None for p in ptr], info.ctypes.data)
            self.info = info[0]
        else:
            self.info = ix.locate(*rp, m, align, frames_cap, *ptr)
            self.ret = int(self.info["status"])

    def host(self):
        """(the seven arrays, the spans) as numpy arrays of k_alloc and m entries."""
        import cairo_zstd_amd as cz
        arr = [t.cpu().numpy()[:self.k_alloc * np.dtype(ty).itemsize].view(ty) for t, ty in zip(self.d_arr, self.TYPES)]
        return arr, self.d_spans.cpu().numpy()[:self.m * SPAN].view(cz.SEEKABLE_SPAN_DTYPE)


@pytest.mark.parametrize("via", ("c", "py"))
def test_locate_cases_on_the_device(cz, ctx, via):
    """Fails without the feature: the entry points do not exist.  Every locate case of the emulator's, several locates on one index,
    the stream overwritten once the index stands."""
    for name, c in locate_cases().items():
        c.blob                                                          # (resolves what the model wants of every call)
        t, p = stage(c.stream, residue=1 + len(name) % 16)
        if via == "c":
            tab, h = np.zeros(1, dtype=cz.SEEKABLE_INFO_DTYPE), cz.C.c_void_p()
            assert cz.lib().cz_seekable_index_create_device(ctx._h, p, len(c.stream), cz.C.byref(h), tab.ctypes.data) == 0, name
            ix, tab = h, tab[0]
        else:
            ix = ctx.seekable_index(p, len(c.stream))
            tab = ix.info
        assert all(int(tab[k]) == v for k, v in c.inf.items()) and int(tab["detail"]) == 0, name
        t.fill_(0xEE)                                                   # the stream need not outlive the call
        for q, call in enumerate(c.calls):
            got = Located(cz, ix, call.ranges, call.align, call.cap, call.k, call.arrays, via)
            arrays, spans = got.host()
            check_call(name, q, call, got.ret, got.info, 1, arrays, spans)
        if via == "c":
            cz.lib().cz_seekable_index_destroy(ix)
        else:
            ix.close()


def test_index_refuses_a_damaged_table(cz, ctx):
    """Fails without the feature."""
    for reason, c in damaged_cases():
        t, p = stage(c.stream)
        tab, h = np.zeros(1, dtype=cz.SEEKABLE_INFO_DTYPE), cz.C.c_void_p(1)
        assert cz.lib().cz_seekable_index_create_device(ctx._h, p, len(c.stream), cz.C.byref(h), tab.ctypes.data) == model.SEEK_TABLE
        assert not h.value and int(tab[0]["reason"]) == reason and all(int(tab[0][k]) == v for k, v in c.inf.items()), reason
        with pytest.raises(cz.CzError, match=f"reason {reason}"):
            ctx.seekable_index(p, len(c.stream))


@pytest.mark.parametrize("via", ("c", "py"))
def test_gather_cases_on_the_device(cz, ctx, via):
    """Fails without the feature.  Every gather case of the emulator's: the destination at its residue with 0xEE in front of it and
    64 bytes of it behind dst_bytes."""
    import torch
    for name, c in gather_cases().items():
        m, k, n = len(c.ranges), len(c.arrays["out_off"]), len(c.want)
        r = np.array(c.ranges, dtype=np.uint64).reshape(m, 2)
        d_off, d_len = to_device(np.ascontiguousarray(r[:, 0])), to_device(np.ascontiguousarray(r[:, 1]))
        d_out_off, d_content_off = (to_device(np.array(c.arrays[x], dtype=np.uint64)) for x in ("out_off", "content_off"))
        d_dec, d_spans = to_device(np.frombuffer(c.decoded, dtype=np.uint8)), to_device(c.spans)
        d_blk = torch.full((c.residue + n + 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        args = (d_dec.data_ptr(), d_out_off.data_ptr(), d_content_off.data_ptr(), k, d_off.data_ptr(), d_len.data_ptr(), d_spans.data_ptr(), m,
                d_blk.data_ptr() + c.residue, n)
        if via == "c":
            assert cz.lib().cz_seekable_gather_device(ctx._h, *args) == 0, name
        else:
            ctx.seekable_gather_device(*args)
        ctx.synchronize()
        block = d_blk.cpu().numpy().tobytes()
        check_gathered(name, c, block)
        assert len(block) == c.residue + n + 64


def test_argument_refusals_on_the_host(cz, ctx):
    """Fails without the feature.  Decided on the host, nothing launched: every refusal is a status."""
    import torch
    L, INVALID = cz.lib(), model.INVALID_ARG
    sizes = [5, 0, 9]
    stream = fmt.build([b"a", b"b", b"c"], sizes)
    t, p = stage(stream)
    ix = ctx.seekable_index(p, len(stream))
    d = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    q = d.data_ptr()
    info = np.zeros(1, dtype=cz.SEEKABLE_READ_INFO_DTYPE)
    none8 = [None] * 8
    for align in (0, 3, 48, 8192):
        assert L.cz_seekable_locate_device(ix._h, q, q, 1, align, 0, *none8, info.ctypes.data) == INVALID == int(info[0]["status"]), align
    assert L.cz_seekable_locate_device(None, q, q, 1, 1, 0, *none8, info.ctypes.data) == INVALID
    assert L.cz_seekable_locate_device(ix._h, q, q, 1, 1, 0, *none8, None) == INVALID
    assert L.cz_seekable_locate_device(ix._h, q, q, model.MAX_RANGES + 1, 1, 0, *none8, info.ctypes.data) == INVALID
    assert L.cz_seekable_locate_device(ix._h, None, q, 1, 1, 0, *none8, info.ctypes.data) == INVALID
    assert L.cz_seekable_locate_device(ix._h, q, None, 1, 1, 0, *none8, info.ctypes.data) == INVALID
    assert L.cz_seekable_locate_device(ix._h, None, None, 0, 4096, 0, *none8, info.ctypes.data) == 0      # m = 0 needs no ranges
    assert (int(info[0]["frames"]), int(info[0]["content_bytes"]), int(info[0]["selected"])) == (3, 14, 0)
    tab, h = np.zeros(1, dtype=cz.SEEKABLE_INFO_DTYPE), cz.C.c_void_p(1)
    assert L.cz_seekable_index_create_device(None, p, len(stream), cz.C.byref(h), tab.ctypes.data) == INVALID and not h.value
    assert L.cz_seekable_index_create_device(ctx._h, p, len(stream), None, tab.ctypes.data) == INVALID
    assert L.cz_seekable_index_create_device(ctx._h, p, len(stream), cz.C.byref(h), None) == INVALID
    assert L.cz_seekable_index_create_device(ctx._h, None, len(stream), cz.C.byref(h), tab.ctypes.data) == INVALID
    assert L.cz_seekable_gather_device(None, q, q, q, 1, q, q, q, 1, q, 1) == INVALID
    assert L.cz_seekable_gather_device(ctx._h, q, q, q, 1, q, q, q, model.MAX_RANGES + 1, q, 1) == INVALID
    for hole in range(10):
        if hole in (3, 7, 9):
            continue
        a = [q, q, q, 1, q, q, q, 1, q, 1]
        a[hole] = None
        assert L.cz_seekable_gather_device(ctx._h, *a) == INVALID, hole
    assert L.cz_seekable_gather_device(ctx._h, q, q, q, 0, q, q, q, 1, q, 1) == INVALID                    # bytes to copy and no frame
    assert L.cz_seekable_gather_device(ctx._h, None, None, None, 0, None, None, None, 0, None, 0) == 0     # nothing to do
    assert L.cz_seekable_gather_device(ctx._h, None, None, None, 0, q, q, q, 1, None, 0) == 0
    ix.close()
    L.cz_seekable_index_destroy(None)


def device_read(cz, dctx, d_stream, stream_len, ranges, align=16, ix=None):
    """index (unless given) -> sizing locate -> locate -> ONE decode_batch_device -> gather, all on `dctx`: (info, arrays and spans on
    the host, the decode's result records, the gathered bytes, 64 bytes of poison behind them)."""
    import torch
    own = ix is None
    if own:
        ix = dctx.seekable_index(d_stream.data_ptr(), stream_len)
    size = Located(cz, ix, ranges, align, 0, 0, False, "py")
    assert size.ret == 0
    k, n = int(size.info["selected"]), int(size.info["dst_bytes"])
    loc = Located(cz, ix, ranges, align, k, k, True, "py")
    assert loc.ret == 0 and loc.info.tobytes() == size.info.tobytes()
    d_out = torch.full((int(loc.info["out_bytes"]) + 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
    d_res = torch.zeros(max(k, 1) * cz.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    d_dst = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    a = [t.data_ptr() for t in loc.d_arr]                               # frame, in_off, in_len, out_off, out_cap, checksum, content_off
    if k:
        dctx.decode_batch_device(d_stream.data_ptr(), a[1], a[2], k, d_out.data_ptr(), a[3], a[4], d_res.data_ptr())
    dctx.seekable_gather_device(d_out.data_ptr(), a[3], a[6], k, loc.d_off.data_ptr(), loc.d_len.data_ptr(), loc.d_spans.data_ptr(), len(ranges),
                                d_dst.data_ptr(), n)
    dctx.synchronize()
    if own:
        ix.close()
    arrays, spans = loc.host()
    dst = d_dst.cpu().numpy()
    assert (dst[n:] == 0xEE).all()
    return loc.info, arrays, spans, d_res.cpu().numpy().view(cz.RESULT_DTYPE)[:k], dst[:n].tobytes()


def record_ranges(bufs, m, seed):
    """m seeded ranges over the records' concatenation: whole records, 64-byte slices, slices across two and three records,
    duplicates and empties."""
    rng = np.random.default_rng(seed)
    lens = np.array([len(b) for b in bufs])
    at = np.concatenate([[0], np.cumsum(lens)])
    out = []
    for j in range(m):
        i = int(rng.integers(0, len(bufs) - 2))
        kind = j % 6
        if kind == 0:
            out.append((int(at[i]), int(lens[i])))
        elif kind == 1:
            out.append((int(at[i]) + int(rng.integers(0, max(int(lens[i]) - 64, 1))), min(64, int(lens[i]))))
        elif kind == 2:
            out.append((int(at[i + 1]) - 5, 11))
        elif kind == 3:
            out.append((int(at[i + 1]) - 3, int(lens[i + 1]) + 6))
        elif kind == 4:
            out.append(out[int(rng.integers(0, len(out)))])
        else:
            out.append((int(at[i]) + 1, 0))
    return [(o, min(n, int(at[-1]) - o)) for o, n in out]


@pytest.fixture(scope="module")
def records_stream(cz, ctx):
    bufs = [b for _, b in dr.records(1000, seed=11)]
    assert len(bufs) == 4000
    res, info, packed = compress_and_pack(cz, ctx, bufs, records=True)
    return bufs, res, packed


def test_records_compress_pack_index_locate_decode_gather(cz, ctx, records_stream):
    """Fails without the feature.  4 000 records compressed and packed with checksums, then 500 ranges read on the same context with
    the checksums verified: the bytes, the selection against the model, the calculated checksums against the table's."""
    bufs, res, packed = records_stream
    ranges = record_ranges(bufs, 500, seed=5)
    t, p = stage(packed, residue=0)
    ctx.set_verify_checksum(True)
    try:
        info, arrays, spans, dres, got = device_read(cz, ctx, t, len(packed), ranges)
    finally:
        ctx.set_verify_checksum(False)
    winfo, warrays, wspans = model.locate(packed, ranges, 16)
    assert {k: int(info[k]) for k in winfo} == winfo
    assert [a.tolist() for a in arrays] == [warrays[k] for k in model.ARRAYS] and [tuple(int(x) for x in sp) for sp in spans] == wspans
    assert got == model.gathered(bufs, ranges)
    k = int(info["selected"])
    assert 0 < k == len(warrays["frame"]) < 4000
    assert (dres["status"] == 0).all() and (dres["flags"] & cz.RESULT_CHECKSUM_MATCH).all()
    assert dres["calculated_checksum"].tolist() == arrays[5].tolist() == [int(res[f]["checksum"]) for f in arrays[0]]


def test_fast_split_frames_and_an_empty_input(cz, ctx):
    """Fails without the feature.  Three frames of 300 KiB and an empty one: 200 ranges of up to 4 KiB."""
    import compress_edges as ce
    pool = ce.corpus_text(64 << 10) * 7
    bufs = [pool[101 * i + 1: 101 * i + 1 + (300 << 10)] for i in range(3)] + [b""]
    res, info, packed = compress_and_pack(cz, ctx, bufs, fast_split=True)
    rng = np.random.default_rng(9)
    content = sum(map(len, bufs))
    ranges = [(int(o), int(min(ln, content - o))) for o, ln in zip(rng.integers(0, content + 1, 200), rng.integers(0, 4097, 200))]
    ranges[7] = ((300 << 10) - 2000, 4096)                              # across the first two frames
    t, p = stage(packed, residue=0)
    info, arrays, spans, dres, got = device_read(cz, ctx, t, len(packed), ranges, align=256)
    assert int(info["selected"]) <= 3 and arrays[0].tolist() == model.locate(packed, ranges, 256)[1]["frame"]
    assert (dres["status"] == 0).all() and got == model.gathered(bufs, ranges)


def test_read_seekable_is_slicing_decode_seekable(cz, ctx, records_stream):
    """Fails without the feature."""
    bufs, res, packed = records_stream
    whole = b"".join(cz.decode_seekable(packed, ctx))
    ranges = record_ranges(bufs, 300, seed=6)
    want = [whole[o:o + n] for o, n in ranges]
    assert cz.read_seekable(packed, ctx, ranges) == want
    assert cz.read_seekable(packed, ctx, ranges, verify=True) == want
    assert cz.read_seekable(packed, ctx, []) == [] and cz.read_seekable(packed, ctx, [(0, 0), (len(whole), 0)]) == [b"", b""]
    t, p = stage(packed, residue=0)
    ix = ctx.seekable_index(p, len(packed))
    assert cz.read_seekable(ix, ctx, ranges[:50], stream=t) == want[:50] == cz.read_seekable(ix, ctx, ranges[:50], verify=True, stream=t)
    ix.close()
    with pytest.raises(cz.CzError):
        cz.read_seekable(packed, ctx, [(len(whole), 1)])
    with pytest.raises(cz.CzError):
        cz.read_seekable(packed[:-1], ctx, ranges)


def test_read_seekable_verify_names_the_frame_with_the_wrong_checksum(cz, ctx, records_stream):
    """Fails without the feature.  One checksum of the table is wrong: a read raises for that frame when a range touches it, and
    only then, and only with verify."""
    bufs, res, packed = records_stream
    reason, ents = fmt.parse(packed)
    assert reason == 0
    bad = 1234
    table = len(packed) - 17 - 12 * len(ents)
    spoiled = bytearray(packed)
    spoiled[table + 8 + 12 * bad + 8] ^= 1
    spoiled = bytes(spoiled)
    at = sum(len(b) for b in bufs[:bad])
    touching, beside = [(at - 3, 10), (0, 5)], [(at - 30, 30), (at + len(bufs[bad]), 8), (0, 5)]
    content = b"".join(bufs)
    assert cz.read_seekable(spoiled, ctx, beside, verify=True) == [content[o:o + n] for o, n in beside]
    assert cz.read_seekable(spoiled, ctx, touching) == [content[o:o + n] for o, n in touching]
    with pytest.raises(cz.CzError, match=f"frame {bad}:"):
        cz.read_seekable(spoiled, ctx, touching, verify=True)


def test_pack_and_open_are_unchanged_around_a_read(cz, ctx):
    """The packed stream and the opened arrays of a fixed batch before and after an index, a locate and a gather on the same context.
    Passes without the feature up to the read in the middle, which does not exist there."""
    import torch
    bufs = [b for _, b in dr.records(20, seed=3)]

    def pack_and_open():
        res, info, packed = compress_and_pack(cz, ctx, bufs, records=True)
        t, p = stage(packed, residue=0)
        k = len(bufs)
        desc = torch.zeros((4, k), dtype=torch.int64, device="cuda:0")
        d_sum = torch.zeros(k, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        inf = ctx.seekable_open_device(p, len(packed), 0, None, 256, desc[0].data_ptr(), desc[1].data_ptr(), desc[2].data_ptr(), desc[3].data_ptr(),
                                       d_sum.data_ptr())
        return packed, inf.tobytes(), desc.cpu().numpy().tobytes(), d_sum.cpu().numpy().tobytes()

    before = pack_and_open()
    t, p = stage(before[0], residue=0)
    ranges = record_ranges(bufs, 40, seed=4)
    info, arrays, spans, dres, got = device_read(cz, ctx, t, len(before[0]), ranges)
    assert got == model.gathered(bufs, ranges)
    assert pack_and_open() == before
