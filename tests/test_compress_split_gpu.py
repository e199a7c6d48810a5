"""CZ_COMPRESS_SPLIT on the MI355X (cz_compress_plan_kernel, cz_compress_segments_kernel): the cases of test_emu_encode_split.py at
the product segment size through cz_compress_batch_device, frames decoded by the oracle and by this library's decoder (single launch
and the pre-pass pipeline with checksums verified), host path = device path, and what only the GPU shows: more units than workgroups,
with identical bytes whatever the batch, the order and the run.  Run with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import compress_frames as cf
from compress_split import blocks_of, first_offset_code, text

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


@pytest.fixture(scope="module")
def S(cz):
    s = cz.compress_split_segment()
    assert s % BLOCK == 0 and BLOCK <= s <= 1 << 20
    return s


def untouched(region, start):
    """Every byte of `region` from `start` on is still the poison."""
    return bool((np.frombuffer(region, dtype=np.uint8)[start:] == POISON).all())


def device_compress(cz, ctx, bufs, caps=None, in_shift=3, checksum=False, split=True):
    """Through cz_compress_batch_device with torch buffers: inputs at odd offsets, output regions poisoned (with the gaps between
    them checked).  Returns [(result, whole region)]."""
    import torch
    lens = [len(b) for b in bufs]
    in_off = np.cumsum([in_shift] + [n + 1 for n in lens[:-1]]).astype(np.uint64)
    host_in = np.zeros(int(in_off[-1]) + lens[-1] + 16, dtype=np.uint8)
    for o, b in zip(in_off, bufs):
        host_in[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    caps = [cz.compress_bound(n) for n in lens] if caps is None else caps
    out_off = np.cumsum([5] + [c + 3 for c in caps[:-1]]).astype(np.uint64)
    total = int(out_off[-1]) + caps[-1] + 64
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(host_in).to(dev)
    d_out = torch.full((total,), POISON, dtype=torch.uint8, device=dev)
    desc = torch.from_numpy(np.stack([in_off, np.array(lens, dtype=np.uint64), out_off, np.array(caps, dtype=np.uint64)]).view(np.int64)).to(dev)
    d_res = torch.zeros(len(bufs) * 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.compress_batch_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(bufs), d_out.data_ptr(), desc[2].data_ptr(),
                              desc[3].data_ptr(), d_res.data_ptr(), checksum=checksum, split=split)
    ctx.synchronize()
    out = d_out.cpu().numpy()
    res = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)
    assert (out[:int(out_off[0])] == POISON).all()
    ends = out_off + np.array(caps, dtype=np.uint64)
    for i in range(len(bufs) - 1):                                      # the 3-byte gaps between regions
        assert (out[int(ends[i]):int(out_off[i + 1])] == POISON).all(), i
    assert (out[int(ends[-1]):] == POISON).all()
    return [(res[i], out[int(out_off[i]):int(out_off[i]) + caps[i]].tobytes()) for i in range(len(bufs))]


def frames_of(cz, S, bufs, got, checksum=False):
    """The frames of `got`, each checked: status, bound, poison past bytes_written, record, Last_Block on the final block only."""
    frames = []
    for i, (b, (r, region)) in enumerate(zip(bufs, got)):
        n = int(r["bytes_written"])
        assert int(r["status"]) == 0, (i, int(r["status"]))
        assert n <= cz.compress_bound(len(b))
        assert untouched(region, n), f"frame {i}: bytes past bytes_written were touched"
        assert int(r["bytes_read"]) == len(b) and int(r["blocks"]) == max(1, -(-len(b) // BLOCK)), i
        assert int(r["flags"]) == (cz.COMPRESS_CHECKSUM if checksum else 0) | (cz.COMPRESS_SPLIT if len(b) > S else 0), i
        _, blocks = blocks_of(region[:n])
        assert [last for _, last, _, _, _ in blocks] == [0] * (len(blocks) - 1) + [1] and len(blocks) == int(r["blocks"]), i
        frames.append(region[:n])
    return frames


def decode_all(cz, bufs, frames, checksum=False):
    """The oracle, then this library's decoder: the single launch and the pre-pass pipeline with checksums verified."""
    import oracle
    for i, (b, fr) in enumerate(zip(bufs, frames)):
        st, out, info = oracle.decode_frame(fr, cap=len(b) + 64)
        assert st == 0 and out == b and info["consumed"] == len(fr) and info["content_size"] == len(b), i
        if checksum:
            assert info["has_checksum"] and info["checksum"] == oracle.xxh64(b) & 0xFFFFFFFF, i
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


def round_trip(cz, ctx, bufs, frames):
    dec = cz.decode_batch_host(frames, [len(b) for b in bufs], ctx)
    assert all(int(r["status"]) == 0 and o == b for (r, o), b in zip(dec, bufs))


def test_up_to_one_segment_is_the_plain_frame(cz, ctx, S):
    T = text(S)
    bufs = [b"", b"\x41", T[:S - 1], T]
    for checksum in (False, True):
        split = frames_of(cz, S, bufs, device_compress(cz, ctx, bufs, checksum=checksum), checksum)
        plain = frames_of(cz, S, bufs, device_compress(cz, ctx, bufs, checksum=checksum, split=False), checksum)
        assert split == plain


def test_split_text_frames(cz, ctx, S):
    """S + 1, 2 S and 2 S + 70 001 bytes: the first segment is the plain frame's, and the frame is no larger than the plain frames of
    its segments together; all decoders read it; the host path gives the same bytes."""
    T = text(2 * S + 70001)
    bufs = [T[:S + 1], T[:2 * S], T]
    split = frames_of(cz, S, bufs, device_compress(cz, ctx, bufs))
    plain = frames_of(cz, 1 << 40, bufs, device_compress(cz, ctx, bufs, split=False))
    pieces = [T[:S], T[S:S + 1], T[S:2 * S], T[2 * S:]]
    p0, p1a, p1b, p2 = (len(r[1][:int(r[0]["bytes_written"])]) for r in device_compress(cz, ctx, pieces, split=False))
    for b, fs, fp, floor in zip(bufs, split, plain, (p0 + p1a, p0 + p1b, p0 + p1b + p2)):
        (hl, bs), (hlp, _) = blocks_of(fs), blocks_of(fp)
        seg0 = bs[S // BLOCK][0]                                        # header and the blocks of segment 0
        assert hl == hlp and fs[:seg0] == fp[:seg0]
        assert len(fs) <= floor, (len(b), len(fs), floor)
    decode_all(cz, bufs, split)
    assert [fr for _, fr in cz.compress_batch_host(bufs, ctx, split=True)] == split
    assert cz.compress(bufs[2], ctx, split=True) == split[2]


def test_rle_raw_history_and_explicit_first_offset(cz, ctx, S):
    rng = np.random.default_rng(99)
    nb = S // BLOCK
    period = bytearray(rng.bytes(1000) * (2 * S // 1000 + 6))[:2 * S + 5000]
    for k in (1, 2):                                                    # a byte that breaks the period right behind each cut
        period[k * S + 2] ^= 0x55
    bufs = [b"\0" * (3 * S), rng.bytes(2 * S), rng.bytes(S) + text(40000, skip=123), bytes(period)]
    got = device_compress(cz, ctx, bufs)
    zeros, rnd, rnd_text, per = frames_of(cz, S, bufs, got)
    assert [t for t, _ in cf.walk(zeros)] == ["rle"] * (3 * nb)
    assert [t for t, _ in cf.walk(rnd)] == ["raw"] * (2 * nb)
    assert [t for t, _ in cf.walk(rnd_text)] == ["raw"] * nb + ["compressed"]
    plain = frames_of(cz, 1 << 40, bufs[3:], device_compress(cz, ctx, bufs[3:], split=False))[0]
    (_, bs), (_, bp) = blocks_of(per), blocks_of(plain)
    assert all(b[2] == 2 for b in bs + bp)
    for k in (1, 2):                                                    # the unsplit frame repeats the offset; a later segment cannot
        assert first_offset_code(plain[bp[k * nb][0]:bp[k * nb][0] + bp[k * nb][4]]) == 0
        assert first_offset_code(per[bs[k * nb][0]:bs[k * nb][0] + bs[k * nb][4]]) == 9
    decode_all(cz, bufs, [zeros, rnd, rnd_text, per])


def test_checksum(cz, ctx, S):
    import oracle
    T = text(2 * S + 70001, skip=4242)
    bufs = [T[:S + 1], T, b"", T[:3000], b"\0" * S + T[:S + 5000]]
    got = device_compress(cz, ctx, bufs, checksum=True)
    frames = frames_of(cz, S, bufs, got, checksum=True)
    for b, (r, _) in zip(bufs, got):
        assert int(r["checksum"]) == oracle.xxh64(b) & 0xFFFFFFFF
    decode_all(cz, bufs, frames, checksum=True)
    assert [fr for _, fr in cz.compress_batch_host(bufs, ctx, checksum=True, split=True)] == frames


def test_output_too_small_is_a_block_aligned_prefix(cz, ctx, S):
    capin = b"\0" * S + text(S, skip=777) + text(5000, skip=31)         # 3 segments
    small = text(3000, skip=5)
    bufs = [capin, small, capin]
    full, neighbour, _ = frames_of(cz, S, bufs, device_compress(cz, ctx, bufs))
    _, blocks = blocks_of(full)
    nb = S // BLOCK
    inside = blocks[nb][0] + (blocks[2 * nb][0] - blocks[nb][0]) // 2   # ends inside segment 1
    placed_inside = max(k for k in range(len(blocks)) if blocks[k][0] <= inside)
    caps = [len(full) - 1, cz.compress_bound(len(small)), inside]
    got = device_compress(cz, ctx, bufs, caps=caps)
    for (r, region), placed in ((got[0], len(blocks) - 1), (got[2], placed_inside)):
        assert int(r["status"]) == cz.status.CZ_E_OUTPUT_TOO_SMALL
        w = int(r["bytes_written"])
        assert w == blocks[placed][0] and region[:w] == full[:w]        # header and the whole blocks placed
        assert int(r["blocks"]) == placed and int(r["bytes_read"]) == placed * BLOCK
        assert untouched(region, w)
        assert int(r["flags"]) == cz.COMPRESS_SPLIT
    assert nb <= placed_inside < 2 * nb
    rn, regn = got[1]
    assert int(rn["status"]) == 0 and regn[:int(rn["bytes_written"])] == neighbour and untouched(regn, len(neighbour))


def test_more_units_than_workgroups_same_bytes_every_way(cz, ctx, S):
    """300 buffers of S + 1 .. 2 S + 5 bytes mixed with 100 short ones: alone, reversed with another input shift, inside a larger
    batch and twice in a row.  The bytes never depend on the batch, the grid or timing."""
    rng = np.random.default_rng(2024)
    pool = text(4 * S + 300_000)
    lens = np.concatenate([np.linspace(S + 1, 2 * S + 5, 300).astype(np.int64), rng.integers(0, 5000, 100)])
    rng.shuffle(lens)
    bufs = [pool[int(o):int(o) + int(n)] for o, n in zip(rng.integers(0, len(pool) - 2 * S - 5, len(lens)), lens)]
    alone = frames_of(cz, S, bufs, device_compress(cz, ctx, bufs))
    again = frames_of(cz, S, bufs, device_compress(cz, ctx, bufs))
    rev = frames_of(cz, S, bufs[::-1], device_compress(cz, ctx, bufs[::-1], in_shift=1))[::-1]
    extra = [pool[int(o):int(o) + 3 * S + 17] for o in rng.integers(0, 100_000, 40)]
    big = extra[:20] + bufs + extra[20:]
    whole = frames_of(cz, S, big, device_compress(cz, ctx, big, in_shift=2))[20:20 + len(bufs)]
    assert alone == again == rev == whole
    assert sum(-(-len(b) // S) for b in bufs) > 700                     # units; the grid is one or two workgroups per CU (256 CUs)
    round_trip(cz, ctx, bufs, alone)


def test_sixteen_segments_round_trip_and_beat_their_pieces(cz, ctx, S):
    big = text(16 * S, skip=1000)
    fr, = frames_of(cz, S, [big], device_compress(cz, ctx, [big]))
    pieces = [big[k * S:(k + 1) * S] for k in range(16)]
    floor = sum(int(r["bytes_written"]) for r, _ in device_compress(cz, ctx, pieces, split=False))
    print(f"16 S = {len(big)}: split frame {len(fr)}, its segments as plain frames {floor}")
    assert len(fr) < floor
    decode_all(cz, [big], [fr])


def test_unknown_flag_and_dictionaries_refuse(cz, ctx):
    import torch
    d = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    p = d.data_ptr()
    L = cz.lib()
    assert L.cz_compress_batch_device(ctx._h, p, p, p, 1, p, p, p, 8, p) == cz.status.CZ_E_INVALID_ARG
    assert L.cz_compress_batch_device(ctx._h, p, p, p, 1, p, p, p, 8 | cz.COMPRESS_SPLIT, p) == cz.status.CZ_E_INVALID_ARG
    assert L.cz_compress_batch_dict_device(ctx._h, p, p, p, 1, p, p, p, cz.COMPRESS_SPLIT, p, p) == cz.status.CZ_E_INVALID_ARG
    h = np.zeros(64, dtype=np.uint64)
    hp = h.ctypes.data
    assert L.cz_compress_batch_host(ctx._h, hp, 8, hp, hp, 1, hp, 64, hp, hp, 8, hp) == cz.status.CZ_E_INVALID_ARG
    assert L.cz_compress_batch_dict_host(ctx._h, hp, 8, hp, hp, 1, hp, 64, hp, hp, cz.COMPRESS_SPLIT, hp, hp) == cz.status.CZ_E_INVALID_ARG
    ctx.synchronize()
    assert (d.cpu().numpy() == 0).all()
