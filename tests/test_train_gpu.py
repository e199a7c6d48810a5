"""cz_dictionary_train_* on the MI355X: the device's dictionaries equal the emulator's (sha256 manifest), the host path's and a
second call's; dictionaries trained on 600 records of each family close the loop train -> compress -> decode (this library, the
oracle, libzstd), with every sequences section in Repeat mode; the size against no dictionary, against another family's dictionary
and against the golden ZDICT dictionaries.  Run with `pytest -m gpu`."""
import hashlib
import json
import os

import numpy as np
import pytest

import dict_frames as dfr
import dict_records as dr
import train_data as td

pytestmark = pytest.mark.gpu
POISON = 0xEE
MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train", "manifest.json")
CAPACITY = 8192


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


def device_train(cz, ctx, samples, capacity, **kw):
    """Through cz_dictionary_train_device with torch buffers: samples at odd offsets, the output region poisoned and in the middle
    of a larger one.  Returns (the dictionary or the CzError's code, the whole region)."""
    import torch
    lens = [len(b) for b in samples]
    off = np.cumsum([3] + [n + 1 for n in lens[:-1]]).astype(np.uint64)
    host = np.zeros(int(off[-1]) + lens[-1] + 16, dtype=np.uint8)
    for o, b in zip(off, samples):
        host[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(host).to(dev)
    desc = torch.from_numpy(np.stack([off, np.array(lens, dtype=np.uint64)]).view(np.int64)).to(dev)
    d_out = torch.full((capacity + 128,), POISON, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    try:
        n = ctx.train_dictionary_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(samples), d_out.data_ptr() + 64, capacity, **kw)
    except cz.CzError as e:
        n = -e.code
    out = d_out.cpu().numpy()
    assert set(out[:64].tolist()) == {POISON} and set(out[64 + max(n, 0):].tolist()) == {POISON}, "bytes outside the dictionary were touched"
    return (out[64:64 + n].tobytes() if n >= 0 else n), out


def test_device_dictionaries_equal_the_emulators(cz, ctx):
    m = json.load(open(MANIFEST))
    inputs = td.manifest_inputs()
    assert sorted(m) == sorted(inputs)
    for name, (samples, cap) in inputs.items():
        raw, _ = device_train(cz, ctx, samples, cap)
        assert (len(raw), hashlib.sha256(raw).hexdigest()) == (m[name]["len"], m[name]["sha256"]), name
        assert cz.train_dictionary(samples, cap, ctx) == raw, name       # the host path
        assert device_train(cz, ctx, samples, cap)[0] == raw, name       # again
        td.check_valid(raw, cap)


def test_argument_errors_write_nothing(cz, ctx):
    ok = [b"a sample of more than eight bytes"] * 4
    assert device_train(cz, ctx, ok, 1023)[0] == -901
    assert device_train(cz, ctx, [b"1234567", b"", b"abc"], 2048)[0] == -901
    assert device_train(cz, ctx, ok, 2048, segment_len=15)[0] == -901
    assert device_train(cz, ctx, ok, 2048, segment_len=4097)[0] == -901
    raw, _ = device_train(cz, ctx, ok, 2048, dict_id=77, segment_len=16)
    assert td.check_valid(raw, 2048, dict_id=77)["content"] == b"".join(ok)


@pytest.fixture(scope="module")
def trained(cz, ctx):
    """The four trained dictionaries, the held-out records, and their frames under the trained dictionaries."""
    raws = [cz.train_dictionary(td.family_records(j, 600), CAPACITY, ctx) for j in range(4)]
    for raw in raws:
        td.check_valid(raw, CAPACITY)
    held = dr.records(200, seed=7)
    bufs, idx = [b for _, b in held], [j for j, _ in held]
    ds = [cz.Dictionary(ctx, raw) for raw in raws]
    ctx.set_compress_dictionaries(ds)
    got = cz.compress_batch_host_dict(bufs, idx, ctx)
    assert all(int(r["status"]) == 0 for r, _ in got)
    return raws, ds, bufs, idx, [f for _, f in got]


def test_the_loop_closes(cz, ctx, trained):
    import oracle
    raws, ds, bufs, idx, frames = trained
    try:
        ctx.set_dictionaries(ds)
        got = cz.decode_batch_host(frames, [len(b) + 64 for b in bufs], ctx)
    finally:
        ctx.set_dictionaries([])
    for i, ((r, out), b) in enumerate(zip(got, bufs)):
        assert int(r["status"]) == 0 and out == b, i
    ods = [oracle.Dictionary(raw) for raw in raws]
    compressed = 0
    for i, (f, b) in enumerate(zip(frames, bufs)):
        assert dfr.header_id(f)[1] == ods[idx[i]].info["id"]
        st, out = oracle.decode_frame_with_dict(f, ods[idx[i]], cap=len(b) + 64)
        assert st == 0 and out == b, i
        if dr.libzstd():
            assert dr.zstd_decompress_dict(f, len(b), raws[idx[i]]) == b, i
        for btype, _, nseq, modes in dfr.blocks(f):                      # the dictionary's tables are the ones in use
            if btype == "compressed" and nseq:
                compressed += 1
                assert modes == (3, 3, 3), (i, modes)
    assert compressed >= len(frames) // 2


def test_size(cz, ctx, trained):
    raws, ds, bufs, idx, frames = trained
    per = lambda fr, j: sum(len(f) for f, k in zip(fr, idx) if k == j)
    T = sum(len(f) for f in frames)
    P = sum(len(f) for _, f in cz.compress_batch_host(bufs, ctx))
    try:
        # another family's trained dictionary: more bytes than the family's own
        for shift in (1, 2, 3):
            other = [f for _, f in cz.compress_batch_host_dict(bufs, [(j + shift) % 4 for j in idx], ctx)]
            for j in range(4):
                assert per(frames, j) < per(other, j), (j, shift, per(frames, j), per(other, j))
        golden = [cz.Dictionary(ctx, raw) for raw in dr.dictionaries()]
        ctx.set_compress_dictionaries(golden)
        Z = sum(len(f) for _, f in cz.compress_batch_host_dict(bufs, idx, ctx))
    finally:
        ctx.set_compress_dictionaries(ds)
    print(f"trained T={T} golden ZDICT Z={Z} plain P={P} T/P={T / P:.4f} Z/P={Z / P:.4f} T/Z={T / Z:.4f}")
    assert T <= 0.55 * P, (T, P)
    assert T <= 0.95 * Z, (T, Z)                                        # measured 0.9002, rounded up to the next 0.05
