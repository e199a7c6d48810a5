"""cz_compress_batch_dict_* on the MI355X: a mixed batch of records with their dictionaries, frames without a dictionary and
frames without a Dictionary_ID field is decoded by this library in one batch (cz_context_set_dictionaries), by the oracle and by
libzstd; the device's frames equal the emulator's (sha256 manifest), the plain compressor's for CZ_COMPRESS_NO_DICT, and the host
path's; they do not depend on the batch; per-frame and argument errors; the size bar.  Run with `pytest -m gpu`."""
import hashlib
import json
import os

import numpy as np
import pytest

import compress_frames as cf
import dict_frames as dfr
import dict_records as dr

pytestmark = pytest.mark.gpu
POISON = 0xEE
NO_DICT = 0xFFFFFFFF
MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compress_dict", "manifest.json")


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


@pytest.fixture(scope="module")
def dicts(cz, ctx):
    ds = [cz.Dictionary(ctx, raw) for raw in dr.dictionaries()]
    ctx.set_compress_dictionaries(ds)
    return ds


def device_compress(cz, ctx, bufs, idx, caps=None, checksum=False, dict_id=True, in_shift=0):
    """Through cz_compress_batch_dict_device with torch buffers: inputs at odd offsets (moved by in_shift), output regions poisoned;
    the gaps between the regions must stay poisoned."""
    import torch
    lens = [len(b) for b in bufs]
    in_off = np.cumsum([3 + in_shift] + [l + 1 for l in lens[:-1]]).astype(np.uint64)
    host_in = np.zeros(int(in_off[-1]) + lens[-1] + 16, dtype=np.uint8)
    for o, b in zip(in_off, bufs):
        host_in[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    caps = [cz.compress_bound(l) for l in lens] if caps is None else caps
    out_off = np.cumsum([5] + [c + 3 for c in caps[:-1]]).astype(np.uint64)
    total = int(out_off[-1]) + caps[-1] + 64
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(host_in).to(dev)
    d_out = torch.full((total,), POISON, dtype=torch.uint8, device=dev)
    desc = torch.from_numpy(np.stack([in_off, np.array(lens, dtype=np.uint64), out_off, np.array(caps, dtype=np.uint64)]).view(np.int64)).to(dev)
    d_idx = torch.from_numpy(np.array(idx, dtype=np.uint32).view(np.int32)).to(dev) if idx is not None else None
    d_res = torch.zeros(len(bufs) * 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.compress_batch_dict_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(bufs), d_out.data_ptr(), desc[2].data_ptr(),
                                   desc[3].data_ptr(), d_idx.data_ptr() if d_idx is not None else 0, d_res.data_ptr(), checksum=checksum,
                                   dict_id=dict_id)
    ctx.synchronize()
    out = d_out.cpu().numpy()
    res = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)
    assert set(out[:int(out_off[0])].tolist()) == {POISON}
    ends = [int(o) + c for o, c in zip(out_off, caps)]
    for i, (a, b) in enumerate(zip(ends, [int(o) for o in out_off[1:]] + [total])):
        assert (out[a:b] == POISON).all(), f"the gap behind region {i} was written"
    return [(res[i], out[int(out_off[i]):int(out_off[i]) + caps[i]].tobytes()) for i in range(len(bufs))]


def frames_of(got):
    for r, region in got:
        assert int(r["status"]) == 0
        assert set(region[int(r["bytes_written"]):]) <= {POISON}
    return [region[:int(r["bytes_written"])] for r, region in got]


def test_the_loop_closes(cz, ctx, dicts):
    import oracle
    recs = dr.records(60, seed=21)
    raw = dr.dictionaries()
    sp = [b for _, b in sorted(cf.special_inputs().items())]
    bufs = [b for _, b in recs] + sp
    idx = [j for j, _ in recs] + [NO_DICT] * len(sp)
    with_id = frames_of(device_compress(cz, ctx, bufs, idx, checksum=True))
    no_id = frames_of(device_compress(cz, ctx, [b for _, b in recs[:40]], [0] * 40, dict_id=False))   # all users: dict_a
    frames = with_id + no_id
    want = bufs + [b for _, b in recs[:40]]
    dict_of = [raw[i] if i != NO_DICT else None for i in idx] + [raw[0]] * 40
    try:                                                                # (the decode setting is independent of the compress one)
        ctx.set_dictionaries(dicts, no_id=dicts[0])
        got = cz.decode_batch_host(frames, [len(b) + 64 for b in want], ctx)
    finally:
        ctx.set_dictionaries([])
    for i, ((r, out), b) in enumerate(zip(got, want)):
        assert int(r["status"]) == 0 and out == b, i
    for i, (f, b) in enumerate(zip(frames, want)):
        if dict_of[i] is None:
            st, out, info = oracle.decode_frame(f, cap=len(b) + 64)
        else:
            st, out = oracle.decode_frame_with_dict(f, oracle.Dictionary(dict_of[i]), cap=len(b) + 64)
        assert st == 0 and out == b, i
        if dr.libzstd():
            assert dr.zstd_decompress_dict(f, len(b), dict_of[i]) == b, i
    assert all(dfr.header_id(f) == (0, 0) for f in no_id)


def test_device_frames_equal_the_emulators(cz, ctx, dicts):
    m = json.load(open(MANIFEST))
    bufs, idx = dr.manifest_batch()
    assert len(bufs) == m["n"]
    for flags, want in m["flags"].items():
        flags = int(flags)
        frames = frames_of(device_compress(cz, ctx, bufs, idx, checksum=bool(flags & 1), dict_id=not flags & 2))
        assert [hashlib.sha256(f).hexdigest() for f in frames] == want, flags


def test_no_dict_frames_equal_the_plain_compressor(cz, ctx, dicts):
    bufs = [b for _, b in cf.corpus_originals()] + [b for _, b in sorted(cf.special_inputs().items())]
    got = frames_of(device_compress(cz, ctx, bufs, [NO_DICT] * len(bufs), checksum=True))
    plain = [f for _, f in cz.compress_batch_host(bufs, ctx, checksum=True)]
    assert got == plain


def test_host_path_equals_device_path_and_determinism(cz, ctx, dicts):
    recs = dr.records(50, seed=4)
    bufs, idx = [b for _, b in recs], [j for j, _ in recs]
    dev = frames_of(device_compress(cz, ctx, bufs, idx))
    host = cz.compress_batch_host_dict(bufs, idx, ctx)
    assert [f for _, f in host] == dev
    # another order, another composition, again
    order = list(reversed(range(len(bufs))))[::2]
    extra = [b"padding " * 1000, bytes(range(256)) * 40]
    mixed = frames_of(device_compress(cz, ctx, extra + [bufs[i] for i in order], [NO_DICT, 2] + [idx[i] for i in order]))
    assert mixed[2:] == [dev[i] for i in order]
    assert frames_of(device_compress(cz, ctx, bufs, idx)) == dev
    # NULL index with one dictionary set: every frame uses it
    one = cz.Context(0)
    try:
        d = cz.Dictionary(one, dr.dictionaries()[0])
        one.set_compress_dictionaries([d])
        users = [b for j, b in recs if j == 0]
        assert [f for _, f in cz.compress_batch_host_dict(users, None, one)] == [dev[i] for i, (j, _) in enumerate(recs) if j == 0]
    finally:
        one.close()


def test_per_frame_errors(cz, ctx, dicts):
    bufs = [b"hello hello hello hello", b"abcdefgh" * 30, b"x" * 100]
    got = device_compress(cz, ctx, bufs, [0, 4, NO_DICT])
    assert [int(r["status"]) for r, _ in got] == [0, 901, 0]
    assert int(got[1][0]["bytes_written"]) == 0 and set(got[1][1]) == {POISON}
    empty = cz.Context(0)                                               # an index set when no dictionaries are set
    try:
        got = cz.compress_batch_host_dict(bufs, [0, NO_DICT, 0], empty)
        assert [int(r["status"]) for r, _ in got] == [901, 0, 901]
    finally:
        empty.close()
    # output too small: the status, and nothing past bytes_written
    recs = dr.records(3, seed=8)
    b, i = [x for _, x in recs], [j for j, _ in recs]
    need = [len(f) for f in frames_of(device_compress(cz, ctx, b, i))]
    caps = [max(1, n - 1) for n in need]
    got = device_compress(cz, ctx, b, i, caps=caps)
    for r, region in got:
        assert int(r["status"]) == 900
        assert set(region[int(r["bytes_written"]):]) <= {POISON}


def test_set_compress_dictionaries_arguments(cz, ctx, dicts):
    other = cz.Context(0)
    try:
        foreign = cz.Dictionary(other, dr.dictionaries()[1])
        recs = dr.records(4, seed=9)
        b, i = [x for _, x in recs], [j for j, _ in recs]
        before = frames_of(device_compress(cz, ctx, b, i))
        for bad in ([dicts[0], foreign], [dicts[0], None]):
            with pytest.raises(cz.CzError) as e:
                ctx.set_compress_dictionaries(bad)
            assert e.value.code == 901
        assert frames_of(device_compress(cz, ctx, b, i)) == before       # the previous setting stays
        with pytest.raises(cz.CzError):
            ctx.set_compress_dictionaries([dicts[0]] * 1025)
        assert frames_of(device_compress(cz, ctx, b, i)) == before
        ctx.set_compress_dictionaries([])                                # cleared: every index fails its frame
        got = device_compress(cz, ctx, b[:1], [0])
        assert int(got[0][0]["status"]) == 901
    finally:
        ctx.set_compress_dictionaries(dicts)
        other.close()


def test_size_bar(cz, ctx, dicts):
    recs = dr.records(200)
    bufs, idx = [b for _, b in recs], [j for j, _ in recs]
    total = sum(len(f) for f in frames_of(device_compress(cz, ctx, bufs, idx)))
    plain = sum(len(f) for _, f in cz.compress_batch_host(bufs, ctx))
    assert total <= 0.55 * plain, (total, plain)
    if dr.libzstd():
        raw = dr.dictionaries()
        ref = sum(len(dr.zstd_compress_dict(b, raw[j], 1)) for j, b in recs)
        assert total <= 1.4 * ref, (total, ref)
