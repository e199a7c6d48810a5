"""cz_compress_batch_* on the MI355X: frames round-trip through the oracle and this library's decoder (single launch and the
pre-pass pipeline), the corpus size bar, large and unaligned batches, determinism, per-frame errors, host path = device path.
Run with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import compress_frames as cf

pytestmark = pytest.mark.gpu
POISON = 0xEE


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


def device_compress(cz, ctx, bufs, caps=None, in_shift=3, checksum=False):
    """Through cz_compress_batch_device with torch buffers: inputs at odd offsets, output regions poisoned.
    Returns [(result, whole region)]."""
    import torch
    lens = [len(b) for b in bufs]
    in_off = np.cumsum([in_shift] + [l + 1 for l in lens[:-1]]).astype(np.uint64)
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
    d_res = torch.zeros(len(bufs) * 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.compress_batch_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(bufs), d_out.data_ptr(), desc[2].data_ptr(),
                              desc[3].data_ptr(), d_res.data_ptr(), checksum=checksum)
    ctx.synchronize()
    out = d_out.cpu().numpy()
    res = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)
    assert set(out[:int(out_off[0])].tolist()) == {POISON}
    return [(res[i], out[int(out_off[i]):int(out_off[i]) + caps[i]].tobytes()) for i in range(len(bufs))], out, out_off, caps


def frames_of(got):
    return [region[:int(r["bytes_written"])] for r, region in got]


def test_corpus_round_trip_and_size(cz, ctx):
    import oracle
    names, bufs = zip(*cf.corpus_originals())
    assert len(bufs) == 69
    got = cz.compress_batch_host(list(bufs), ctx)
    frames = []
    for name, b, (r, fr) in zip(names, bufs, got):
        assert int(r["status"]) == 0 and int(r["bytes_read"]) == len(b), name
        assert len(fr) <= cz.compress_bound(len(b))
        st, out, info = oracle.decode_frame(fr, cap=len(b) + 64)
        assert st == 0 and out == b and info["consumed"] == len(fr), name
        if cf.libzstd():
            assert cf.libzstd_decompress(fr, len(b)) == b, name
        frames.append(fr)
    total = sum(len(f) for f in frames)
    print(f"corpus: {sum(map(len, bufs))} -> {total} bytes")
    assert total <= 290_000
    caps = [len(b) + 64 for b in bufs]
    # this library's decoder: the single launch, then the pre-pass pipeline with checksums verified
    for prepass in (False, True):
        dctx = cz.Context(0)
        if prepass:
            dctx.set_chain_arena(64 << 20, min_sequences=0)
            dctx.set_literal_arena(32 << 20)
            dctx.set_verify_checksum(True)
        dec = cz.decode_batch_host(frames, caps, dctx)
        dctx.close()
        for name, b, (r, out) in zip(names, bufs, dec):
            assert int(r["status"]) == 0 and out == b, (name, prepass)


def test_checksum_frames_verify(cz, ctx):
    import oracle
    bufs = [b for _, b in cf.corpus_originals()][::3] + [b""]
    got = cz.compress_batch_host(bufs, ctx, checksum=True)
    dctx = cz.Context(0)
    dctx.set_chain_arena(64 << 20, min_sequences=0)
    dctx.set_literal_arena(32 << 20)
    dctx.set_verify_checksum(True)
    dec = cz.decode_batch_host([fr for _, fr in got], [len(b) + 64 for b in bufs], dctx)
    dctx.close()
    for b, (r, fr), (dr, out) in zip(bufs, got, dec):
        assert int(r["checksum"]) == oracle.xxh64(b) & 0xFFFFFFFF
        assert out == b and dr["flags"] & cz.RESULT_CHECKSUM_MATCH


def test_large_unaligned_batch_keeps_poison(cz, ctx):
    import oracle
    bufs = tiled(2000, 128 << 10, seed=7)
    got, out, out_off, caps = device_compress(cz, ctx, bufs)
    frames = frames_of(got)
    for i, ((r, region), b) in enumerate(zip(got, bufs)):
        n = int(r["bytes_written"])
        assert int(r["status"]) == 0, i
        assert set(region[n:]) <= {POISON}, f"frame {i}: bytes past bytes_written were touched"
    for i in range(len(bufs) - 1):                                      # the 3-byte gaps between regions too
        e = int(out_off[i]) + caps[i]
        assert set(out[e:int(out_off[i + 1])].tolist()) == {POISON}
    for i in range(0, 2000, 97):
        st, dec, info = oracle.decode_frame(frames[i], cap=len(bufs[i]) + 64)
        assert st == 0 and dec == bufs[i], i
    dec = cz.decode_batch_host(frames, [len(b) for b in bufs], ctx)
    assert all(int(r["status"]) == 0 and o == b for (r, o), b in zip(dec, bufs))
    ratio = sum(len(b) for b in bufs) / sum(map(len, frames))
    print(f"2000 x 128 KiB: ratio {ratio:.3f}")


def test_input_beyond_the_window(cz, ctx):
    import oracle
    big = tiled(1, 3 << 20, seed=3)[0]
    got, _, _, _ = device_compress(cz, ctx, [big, b"small"])
    fr = frames_of(got)[0]
    assert not (fr[4] >> 5) & 1                                        # not single-segment: 1 MiB window
    st, out, info = oracle.decode_frame(fr, cap=len(big) + 64)
    assert st == 0 and out == big and info["window_size"] == 1 << 20
    assert len(cf.walk(fr)) == 24


def test_deterministic(cz, ctx):
    bufs = tiled(2000, 128 << 10, seed=11)
    mid = bufs[700:750]
    alone = frames_of(device_compress(cz, ctx, mid)[0])
    rev = frames_of(device_compress(cz, ctx, mid[::-1], in_shift=1)[0])[::-1]
    whole = frames_of(device_compress(cz, ctx, bufs)[0])[700:750]
    assert alone == rev == whole


def test_output_too_small_is_that_frame_only(cz, ctx):
    bufs = [b for _, b in cf.corpus_originals() if len(b) > 1000][:12]
    ref = frames_of(device_compress(cz, ctx, bufs)[0])
    caps = [cz.compress_bound(len(b)) for b in bufs]
    caps[5] = len(ref[5]) - 1
    got, out, out_off, _ = device_compress(cz, ctx, bufs, caps=caps)
    for i, (r, region) in enumerate(got):
        if i == 5:
            assert int(r["status"]) == cz.status.CZ_E_OUTPUT_TOO_SMALL
            assert set(region[int(r["bytes_written"]):]) <= {POISON}
        else:
            assert int(r["status"]) == 0 and region[:int(r["bytes_written"])] == ref[i], i


def test_host_path_matches_device_path(cz, ctx):
    bufs = tiled(64, 200_000, seed=5) + [b"", b"a", b"\x00" * 300000]
    dev = frames_of(device_compress(cz, ctx, bufs)[0])
    host = [fr for _, fr in cz.compress_batch_host(bufs, ctx)]
    assert host == dev
    assert cz.compress(bufs[0], ctx) == dev[0]
