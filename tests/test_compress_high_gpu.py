"""CZ_COMPRESS_HIGH on the MI355X (cz_compress_frames_high_kernel): the flag is accepted alone and with the checksum and refused with
every other level and with dictionaries; the corpus originals decode three ways and come out smaller in total than with
CZ_COMPRESS_FSE_TABLES; the constructed inputs of tests/compress_high.py meet their expectations and their frames are byte for byte
the CPU emulator's (tests/golden/compress_high); a poisoned, unaligned tiled batch; more frames than workgroups; 24 blocks with
offsets up to 1 MiB; host path = device path; and the other levels write what they wrote before a launch of this one.  Every test
fails without the feature: 256 is an unknown bit there.  Run with `pytest -m gpu`."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import compress_edges as ce
import compress_frames as cf
import compress_high as ch
from compress_split import blocks_of
from test_compress_fast_split_gpu import device_compress, frames
from test_compress_fse_gpu import POISON, ctx, cz, decode_three_ways, tiled  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu
HIGH = 256
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compress_high")


def libzstd_total(bufs, level):
    """The sum of libzstd's frame sizes at `level`, or None without libzstd."""
    z = cf.libzstd()
    if z is None:
        return None
    z.ZSTD_compress.restype = ctypes.c_size_t
    z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    z.ZSTD_compressBound.restype = ctypes.c_size_t
    z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    total = 0
    for b in bufs:
        dst = ctypes.create_string_buffer(z.ZSTD_compressBound(len(b)))
        total += z.ZSTD_compress(dst, len(dst), bytes(b), len(b), level)
    return total


def test_flag_is_accepted_alone_and_with_the_checksum_only(cz, ctx):
    import torch
    assert cz.COMPRESS_HIGH == HIGH
    L = cz.lib()
    src = b"abcdabcdabcdabcd-abcdabcdabcdabcd" * 3
    cap = cz.compress_bound(len(src))
    d_in = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).to("cuda:0")
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    desc = torch.tensor([0, len(src), 0, cap], dtype=torch.int64, device="cuda:0")
    d_res = torch.zeros(32, dtype=torch.uint8, device="cuda:0")
    h_in, h_out = np.frombuffer(src, dtype=np.uint8).copy(), np.zeros(cap, dtype=np.uint8)
    h_desc, h_res = np.array([0, len(src), 0, cap], dtype=np.uint64), np.zeros(1, dtype=cz.COMPRESS_RESULT_DTYPE)

    def both(flags):
        st_d = L.cz_compress_batch_device(ctx._h, d_in.data_ptr(), desc[0:].data_ptr(), desc[1:].data_ptr(), 1, d_out.data_ptr(),
                                          desc[2:].data_ptr(), desc[3:].data_ptr(), flags, d_res.data_ptr())
        ctx.synchronize()
        st_h = L.cz_compress_batch_host(ctx._h, h_in.ctypes.data, h_in.size, h_desc[0:].ctypes.data, h_desc[1:].ctypes.data, 1,
                                        h_out.ctypes.data, h_out.size, h_desc[2:].ctypes.data, h_desc[3:].ctypes.data, flags, h_res.ctypes.data)
        return st_d, st_h

    for bit in (4, 16, 32, 64, 128, 8):                                 # refused at the call: nothing is written to zeroed regions
        for flags in (HIGH | bit, HIGH | 1 | bit):
            assert both(flags) == (cz.status.CZ_E_INVALID_ARG, cz.status.CZ_E_INVALID_ARG), flags
    assert not d_out.cpu().numpy().any() and not d_res.cpu().numpy().any() and not h_out.any() and int(h_res[0]["flags"]) == 0
    p, hp = d_res.data_ptr(), h_res.ctypes.data
    for flags in (HIGH, HIGH | 1):
        assert L.cz_compress_batch_dict_device(ctx._h, p, p, p, 1, p, p, p, flags, p, p) == cz.status.CZ_E_INVALID_ARG
        assert L.cz_compress_batch_dict_host(ctx._h, hp, 8, hp, hp, 1, hp, 32, hp, hp, flags, hp, hp) == cz.status.CZ_E_INVALID_ARG
    for flags in (HIGH, HIGH | 1):
        assert both(flags) == (cz.status.CZ_OK, cz.status.CZ_OK), flags
        r = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)[0]
        assert int(r["status"]) == 0 and int(r["flags"]) == flags
        dev = d_out.cpu().numpy()[:int(r["bytes_written"])].tobytes()
        assert int(h_res[0]["status"]) == 0 and int(h_res[0]["flags"]) == flags
        assert h_out[:int(h_res[0]["bytes_written"])].tobytes() == dev
        assert cf.libzstd() is None or cf.libzstd_decompress(dev, len(src)) == src
        assert dev == cz.compress(src, ctx, checksum=bool(flags & 1), high=True)
    for kw in ({"split": True}, {"fse_tables": True}, {"fast": True}, {"records": True}, {"fast_split": True}):
        with pytest.raises(cz.CzError):
            cz.compress(src, ctx, high=True, **kw)


def test_corpus_three_decoders_and_size(cz, ctx):
    names, bufs = zip(*cf.corpus_originals())
    assert len(bufs) == 69
    got = cz.compress_batch_host(list(bufs), ctx, high=True)
    for name, b, (r, fr) in zip(names, bufs, got):
        assert int(r["status"]) == 0 and int(r["bytes_read"]) == len(b) and int(r["flags"]) == HIGH, name
        assert len(fr) <= cz.compress_bound(len(b)), name
    high = [fr for _, fr in got]
    decode_three_ways(cz, list(bufs), high)
    fse = [fr for _, fr in cz.compress_batch_host(list(bufs), ctx, fse_tables=True)]
    a, b = sum(map(len, high)), sum(map(len, fse))
    print(f"69 corpus originals: {a} bytes with CZ_COMPRESS_HIGH, {b} with CZ_COMPRESS_FSE_TABLES; libzstd levels 1, 3, 6: "
          f"{[libzstd_total(bufs, lv) for lv in (1, 3, 6)]}")
    assert a < b


@pytest.fixture(scope="module")
def built():
    return dict(ch.constructed(), two_blocks=(ch.two_blocks(), ch.expect_two_blocks),
                raw_then_compressed=(ch.raw_then_compressed(), ch.expect_raw_then_compressed))


def test_constructed_inputs_and_the_emulators_bytes(cz, ctx, built):
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        manifest = json.load(f)["frames"]
    assert set(manifest) == set(built)
    bufs = [b.data for b, _ in built.values()]
    got = frames(device_compress(cz, ctx, bufs, high=True))
    for (name, (b, expect)), fr in zip(built.items(), got):
        m = manifest[name]
        assert hashlib.sha256(b.data).hexdigest() == m["input_sha256"], f"{name}: the input changed; run {'scripts/gen_compress_high_golden.py'}"
        expect(ce.analyse(fr, b.data), b)
        assert len(fr) == m["len"] and hashlib.sha256(fr).hexdigest() == m["sha256"], f"{name}: not the emulator's frame"
        if m["file"]:
            with open(os.path.join(GOLDEN, m["file"]), "rb") as f:
                assert f.read() == fr, name
    lazy = built["lazy_sites"][0]
    (fse,) = frames(device_compress(cz, ctx, [lazy.data], fse_tables=True))
    ch.expect_lazy_sites(ce.analyse(fse, lazy.data), lazy, high=False)


def test_tiled_batch_keeps_poison_and_is_smaller(cz, ctx):
    batch = tiled(32, 128 << 10, seed=21)
    high = frames(device_compress(cz, ctx, batch, high=True))           # (device_compress checks the poison between the regions)
    fse = frames(device_compress(cz, ctx, batch, fse_tables=True))
    decode_three_ways(cz, batch, high)
    a, b = sum(map(len, high)), sum(map(len, fse))
    print(f"32 x 128 KiB: ratio {sum(map(len, batch)) / a:.3f} with CZ_COMPRESS_HIGH, {sum(map(len, batch)) / b:.3f} with CZ_COMPRESS_FSE_TABLES")
    assert a < b


def test_more_frames_than_workgroups(cz, ctx):
    import oracle
    bufs = tiled(600, 3000, seed=5)
    got = cz.compress_batch_host(bufs, ctx, high=True)
    for b, (r, fr) in zip(bufs, got):
        st, out, _ = oracle.decode_frame(fr, cap=len(b) + 64)
        assert int(r["status"]) == 0 and st == 0 and out == b
    for i in (0, 1, 255, 256, 257, 511, 599):
        assert cz.compress(bufs[i], ctx, high=True) == got[i][1], i


def test_several_blocks(cz, ctx):
    big = tiled(1, 3 << 20, seed=3)[0]
    (fr,) = frames(device_compress(cz, ctx, [big], high=True))
    hl, blocks = blocks_of(fr)
    assert len(blocks) == 24 and [b[1] for b in blocks] == [0] * 23 + [1]
    an = ce.analyse(fr, big)
    assert not an["header"]["single"] and an["header"]["window"] == 1 << 20
    assert max(o for b in an["blocks"] if b["type"] == "compressed" for o in b["offsets"]) <= 1 << 20
    decode_three_ways(cz, [big], [fr])


def test_host_path_matches_device_path(cz, ctx):
    bufs = tiled(6, 128 << 10, seed=21) + [b"", b"a", b"\x00" * 300000, tiled(1, 700_000, seed=9)[0]]
    for checksum in (False, True):
        dev = frames(device_compress(cz, ctx, bufs, high=True, checksum=checksum))
        host = cz.compress_batch_host(bufs, ctx, high=True, checksum=checksum)
        assert all(int(r["status"]) == 0 and int(r["flags"]) == HIGH | checksum for r, _ in host)
        assert [fr for _, fr in host] == dev


def test_other_levels_unchanged_around_a_launch(cz, ctx):
    batch = tiled(8, 128 << 10, seed=21)
    kws = ({}, {"fse_tables": True}, {"fast": True}, {"records": True}, {"fast_split": True})
    small = [b[:20000] for b in batch]

    def run(kw):
        return [fr for _, fr in cz.compress_batch_host(small if "records" in kw else batch, ctx, **kw)]
    before = [run(kw) for kw in kws]
    high = [fr for _, fr in cz.compress_batch_host(batch, ctx, high=True)]
    assert [run(kw) for kw in kws] == before
    assert [fr for _, fr in cz.compress_batch_host(batch, ctx, high=True)] == high
