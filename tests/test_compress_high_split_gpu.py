"""CZ_COMPRESS_HIGH_SPLIT on the MI355X (cz_compress_plan_kernel, cz_compress_segments_high_kernel; S = 512 KiB, W = 512 KiB): the flag
is accepted alone and with the checksum and refused with every other bit and with dictionaries; inputs of at most one segment come
out byte for byte as with CZ_COMPRESS_HIGH; longer ones decode three ways, start with the CZ_COMPRESS_HIGH frame's segment 0, pass the
history model and the reach check of tests/compress_high_split.py per segment and keep offsets within 1 MiB; the frames are smaller
than those of CZ_COMPRESS_SPLIT | CZ_COMPRESS_FSE_TABLES; more units than workgroups, alone, reversed, inside a larger batch and twice
in a row, give identical frames; a 16 MiB buffer; the out_cap sweep; host path = device path; and the other levels write what they
wrote before a launch of this one.  Every test fails without the feature: 512 is an unknown bit there.  Run with `pytest -m gpu`."""
import numpy as np
import pytest

import compress_edges as ce
import compress_frames as cf
import compress_high_split as hs
from compress_split import blocks_of
from test_compress_fast_split_gpu import device_compress, frames
from test_compress_fse_gpu import POISON, ctx, cz, decode_three_ways, tiled  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu
HIGH, HIGH_SPLIT = 256, 512
OK, TOO_SMALL = 0, 900
BLOCK = 128 << 10
W = 512 << 10                   # CZE_OVERLAP of the product build
FIELDS = ("status", "blocks", "bytes_read", "bytes_written", "checksum")


def test_flag_is_accepted_alone_and_with_the_checksum_only(cz, ctx):
    """512 and 513 in cz_compress_batch_device / _host; CZ_E_INVALID_ARG with each of 2, 4, 8, 16, 32, 64, 128 and 256 and in
    cz_compress_batch_dict_*; Python raises on the refused combinations."""
    import torch
    assert cz.COMPRESS_HIGH_SPLIT == HIGH_SPLIT
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

    for bit in (2, 4, 8, 16, 32, 64, 128, 256):                         # refused at the call: nothing is written to zeroed regions
        for flags in (HIGH_SPLIT | bit, HIGH_SPLIT | 1 | bit):
            assert both(flags) == (cz.status.CZ_E_INVALID_ARG, cz.status.CZ_E_INVALID_ARG), flags
    assert not d_out.cpu().numpy().any() and not d_res.cpu().numpy().any() and not h_out.any() and int(h_res[0]["flags"]) == 0
    p, hp = d_res.data_ptr(), h_res.ctypes.data
    for flags in (HIGH_SPLIT, HIGH_SPLIT | 1):
        assert L.cz_compress_batch_dict_device(ctx._h, p, p, p, 1, p, p, p, flags, p, p) == cz.status.CZ_E_INVALID_ARG
        assert L.cz_compress_batch_dict_host(ctx._h, hp, 8, hp, hp, 1, hp, 32, hp, hp, flags, hp, hp) == cz.status.CZ_E_INVALID_ARG
    for flags in (HIGH_SPLIT, HIGH_SPLIT | 1):
        assert both(flags) == (cz.status.CZ_OK, cz.status.CZ_OK), flags
        r = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)[0]
        assert int(r["status"]) == 0 and int(r["flags"]) == flags
        dev = d_out.cpu().numpy()[:int(r["bytes_written"])].tobytes()
        assert int(h_res[0]["status"]) == 0 and int(h_res[0]["flags"]) == flags
        assert h_out[:int(h_res[0]["bytes_written"])].tobytes() == dev
        assert cf.libzstd() is None or cf.libzstd_decompress(dev, len(src)) == src
        assert dev == cz.compress(src, ctx, checksum=bool(flags & 1), high_split=True)
        assert dev == cz.compress(src, ctx, checksum=bool(flags & 1), high=True)
    for kw in ({"split": True}, {"fse_tables": True}, {"fast": True}, {"records": True}, {"fast_split": True}, {"high": True}):
        with pytest.raises(cz.CzError):
            cz.compress(src, ctx, high_split=True, **kw)
        with pytest.raises(cz.CzError):
            cz.compress(src, ctx, high_split=True, checksum=True, **kw)
    with pytest.raises(cz.CzError):
        cz.compress_batch_host_dict([src], None, ctx, high_split=True)


@pytest.mark.parametrize("checksum", (False, True))
def test_up_to_one_segment_is_the_high_frame(cz, ctx, checksum):
    S = cz.compress_split_segment()
    bufs = [b"", b"a", b"\x00" * 300000, tiled(1, 128 << 10, seed=4)[0], tiled(1, S, seed=6)[0]]
    got = device_compress(cz, ctx, bufs, checksum=checksum, high_split=True)
    want = device_compress(cz, ctx, bufs, checksum=checksum, high=True)
    for i, ((r, region), (q, wanted)) in enumerate(zip(got, want)):
        assert [int(r[k]) for k in FIELDS] == [int(q[k]) for k in FIELDS] and int(r["status"]) == OK, i
        assert int(r["flags"]) == HIGH_SPLIT | checksum and int(q["flags"]) == HIGH | checksum, i
        assert region == wanted, f"[{i}]: the output region differs from the high level's"


@pytest.fixture(scope="module")
def boundary(cz, ctx):
    """S + 1, S + 5, 2 S, 2 S + 70 001 and 5 S + 3 bytes: (inputs, frames in a poisoned, unaligned output, the high level's frames)."""
    S = cz.compress_split_segment()
    big = tiled(1, 5 * S + 3, seed=17)[0]
    bufs = [big[:S + 1], big[:S + 5], big[1000:1000 + 2 * S], big[77:77 + 2 * S + 70001], big]
    got = device_compress(cz, ctx, bufs, high_split=True)
    for b, (r, region) in zip(bufs, got):
        n = int(r["bytes_written"])
        assert int(r["status"]) == OK and int(r["flags"]) == HIGH_SPLIT and int(r["bytes_read"]) == len(b)
        assert n <= cz.compress_bound(len(b)) and (np.frombuffer(region, dtype=np.uint8)[n:] == POISON).all()
        assert int(r["blocks"]) == -(-len(b) // BLOCK) == len(blocks_of(region[:n])[1])
    return bufs, frames(got), frames(device_compress(cz, ctx, bufs, high=True))


def test_boundary_batch_decodes_three_ways(cz, boundary):
    bufs, split, _ = boundary
    decode_three_ways(cz, bufs, split)


def test_boundary_batch_segments(cz, boundary):
    """Segment 0 is the CZ_COMPRESS_HIGH frame's; every segment passes the history model; no match reaches in front of the overlap or
    past 1 MiB; every later segment that has sequences starts with an explicit offset."""
    S = cz.compress_split_segment()
    bufs, split, high = boundary
    for b, fs, fh in zip(bufs, split, high):
        (hl, bs), (hh, bh) = blocks_of(fs), blocks_of(fh)
        seg0 = bs[3][0] + bs[3][4]                                      # the header and the four blocks of segment 0
        assert hl == hh and [x[1] for x in bs] == [0] * (len(bs) - 1) + [1]
        assert fs[:seg0] == fh[:seg0], len(b)
        an = ce.analyse(fs, b)
        counts = hs.check_history(an, S)
        hs.check_reach(an, S, W)
        assert len(counts) == -(-len(b) // S)
        assert max(o for blk in an["blocks"] for o in blk.get("offsets", [0])) <= 1 << 20
        for k, first in enumerate(hs.first_sequences(an, S)):
            assert k == 0 or first is None or first[2] > 3, (len(b), k, first)
        print(f"{len(b)} bytes: {len(fs)} split, {len(fh)} unsplit; repeat codes per segment {counts}")


def test_frames_are_smaller_than_split_fse(cz, ctx):
    bufs = tiled(3, 2 << 20, seed=33)
    mine = [fr for _, fr in cz.compress_batch_host(bufs, ctx, high_split=True)]
    other = [fr for _, fr in cz.compress_batch_host(bufs, ctx, split=True, fse_tables=True)]
    whole = [fr for _, fr in cz.compress_batch_host(bufs, ctx, high=True)]
    a, b, c = (sum(map(len, x)) for x in (mine, other, whole))
    print(f"3 x 2 MiB: {a} bytes with CZ_COMPRESS_HIGH_SPLIT, {b} with CZ_COMPRESS_SPLIT | CZ_COMPRESS_FSE_TABLES, {c} with CZ_COMPRESS_HIGH")
    assert a < b


def test_more_units_than_workgroups_alone_reversed_inside_and_twice(cz, ctx):
    """130 buffers of S + 4 097 bytes with the checksum: two segments and a checksum unit each, 390 units.  Alone, reversed, inside a
    larger batch and twice in a row the frames are identical."""
    import oracle
    S = cz.compress_split_segment()
    n = S + 4097
    text = ce.corpus_text(64 << 10)
    pool = text * (n // len(text) + 3)
    bufs = [pool[37 * i + 1: 37 * i + 1 + n] for i in range(130)]
    assert len(set(bufs)) == 130
    alone = device_compress(cz, ctx, bufs, checksum=True, high_split=True)
    assert all(int(r["flags"]) == HIGH_SPLIT | 1 and int(r["blocks"]) == 5 and int(r["checksum"]) == oracle.xxh64(b) & 0xFFFFFFFF
               for b, (r, _) in zip(bufs, alone))
    fr = frames(alone)
    assert frames(device_compress(cz, ctx, bufs, in_shift=1, checksum=True, high_split=True)) == fr      # twice in a row
    assert frames(device_compress(cz, ctx, bufs[::-1], checksum=True, high_split=True))[::-1] == fr
    small = [text[:1], b"", pool[:S], pool[5:5 + 3 * S + 9]]
    inside = frames(device_compress(cz, ctx, small + bufs[:60] + small[::-1] + bufs[60:] + small, in_shift=2, checksum=True, high_split=True))
    assert inside[4:64] + inside[68:138] == fr
    assert inside[:4] == inside[64:68][::-1] == inside[138:]
    for b, f in list(zip(bufs, fr))[::10]:
        st, out, info = oracle.decode_frame(f, cap=len(b) + 64)
        assert st == 0 and out == b and info["has_checksum"] and info["consumed"] == len(f)
    dctx = cz.Context(0)
    dctx.set_verify_checksum(True)
    dec = cz.decode_batch_host(fr, [n + 64] * len(fr), dctx)
    dctx.close()
    for i, (b, (r, out)) in enumerate(zip(bufs, dec)):
        assert int(r["status"]) == 0 and out == b and r["flags"] & cz.RESULT_CHECKSUM_MATCH, i


def test_one_16_mib_buffer_with_the_checksum(cz, ctx):
    import oracle
    big = tiled(1, 16 << 20, seed=5)[0]
    (r, region), = device_compress(cz, ctx, [big], checksum=True, high_split=True)
    assert int(r["status"]) == OK and int(r["bytes_read"]) == len(big) and int(r["blocks"]) == 128 and int(r["flags"]) == HIGH_SPLIT | 1
    assert int(r["checksum"]) == oracle.xxh64(big) & 0xFFFFFFFF
    fr = region[:int(r["bytes_written"])]
    assert len(blocks_of(fr)[1]) == 128
    st, out, info = oracle.decode_frame(fr, cap=len(big) + 64)
    assert st == 0 and out == big and info["has_checksum"] and info["consumed"] == len(fr)
    (q, dec), = cz.decode_batch_host([fr], [len(big) + 64], ctx)
    assert int(q["status"]) == 0 and dec == big


@pytest.mark.parametrize("checksum", (False, True))
def test_out_cap_sweep(cz, ctx, checksum):
    """2 S + 70 001 bytes, nine blocks in three segments: header - 1, header, the end of every block - 1 and exact (among them ends
    inside segment 1 that are no cut), with the checksum full - 1 and full, in one batch next to a frame that fits.  Each frame is
    the whole blocks that fit, a prefix of the full frame, with the poison untouched behind it."""
    S = cz.compress_split_segment()
    b = tiled(1, 2 * S + 70001, seed=8)[0]
    (r, region), = device_compress(cz, ctx, [b], checksum=checksum, high_split=True)
    full = int(r["bytes_written"])
    whole = region[:full]
    hl, blocks = blocks_of(whole)
    assert len(blocks) == 9 and int(r["status"]) == OK
    ends = [at + size for at, _, _, _, size in blocks]
    caps = [hl - 1, hl] + [e - d for e in ends for d in (1, 0)] + ([full - 1, full] if checksum else [])
    bufs = [b] * len(caps) + [b[:S + 7]]
    got = device_compress(cz, ctx, bufs, caps=caps + [cz.compress_bound(S + 7)], checksum=checksum, high_split=True)
    for cap, (q, reg) in zip(caps, got):
        w = int(q["bytes_written"])
        k = sum(1 for e in ends if e <= cap)                            # whole blocks that fit
        assert int(q["flags"]) == HIGH_SPLIT | checksum
        assert reg[:w] == whole[:w] and (np.frombuffer(reg, dtype=np.uint8)[w:] == POISON).all(), cap
        if cap >= full:
            assert (int(q["status"]), int(q["blocks"]), int(q["bytes_read"]), w) == (OK, 9, len(b), full), cap
        elif k == 9:                                                    # every block placed, the checksum does not fit
            assert (int(q["status"]), int(q["blocks"]), int(q["bytes_read"]), w) == (TOO_SMALL, 9, len(b), ends[8]), cap
        else:
            want = ends[k - 1] if k else (hl if cap >= hl else 0)
            assert (int(q["status"]), int(q["blocks"]), int(q["bytes_read"]), w) == (TOO_SMALL, k, k * BLOCK, want), (cap, k)
    assert ends[5] in caps and ends[5] not in (ends[3], ends[7])       # a block boundary inside segment 1 that is no cut
    q, reg = got[-1]
    assert int(q["status"]) == OK and int(q["bytes_read"]) == S + 7


def test_host_path_matches_device_path(cz, ctx, boundary):
    bufs = boundary[0][:4] + [b"", b"a", b"\x00" * 300000]
    for checksum in (False, True):
        dev = frames(device_compress(cz, ctx, bufs, high_split=True, checksum=checksum))
        host = cz.compress_batch_host(bufs, ctx, high_split=True, checksum=checksum)
        assert all(int(r["status"]) == 0 and int(r["flags"]) == HIGH_SPLIT | checksum for r, _ in host)
        assert [fr for _, fr in host] == dev
    assert boundary[1][:4] == [fr for _, fr in cz.compress_batch_host(bufs[:4], ctx, high_split=True)]


def test_other_levels_unchanged_around_a_launch(cz, ctx):
    """Frames of flags 0, 4, 4 | 16, 16, 32, 64, 128 and 256 on the same context, before and after a launch of 512."""
    batch = tiled(6, 128 << 10, seed=21) + tiled(1, 700_000, seed=9)
    kws = ({}, {"split": True}, {"split": True, "fse_tables": True}, {"fse_tables": True}, {"fast": True}, {"records": True},
           {"fast_split": True}, {"high": True})
    small = [b[:20000] for b in batch]

    def run(kw):
        return [fr for _, fr in cz.compress_batch_host(small if "records" in kw else batch, ctx, **kw)]
    before = [run(kw) for kw in kws]
    mine = [fr for _, fr in cz.compress_batch_host(batch, ctx, high_split=True)]
    assert [run(kw) for kw in kws] == before
    assert [fr for _, fr in cz.compress_batch_host(batch, ctx, high_split=True)] == mine
    assert mine[:6] == before[7][:6] and mine[6] != before[7][6]       # one segment: the high level's frame; two: not
