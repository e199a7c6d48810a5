"""CZ_COMPRESS_FAST_SPLIT on the MI355X (cz_compress_fast_plan_kernel, cz_compress_groups_fast_kernel): the flag is accepted alone and
with the checksum and refused with every other bit and with dictionaries; for every input and every out_cap the output region and
the result fields status, blocks, bytes_read, bytes_written and checksum are those of a CZ_COMPRESS_FAST launch of the same batch on
the same context, with flags 128 | checksum; the frames decode under the oracle, libzstd and this library's decoder; more units than
workgroups, alone, reversed, inside a larger batch and twice in a row, give identical frames; host path = device path; and the other
compress kernels write what they wrote before and after a fast-split launch.  Run with `pytest -m gpu`."""
import numpy as np
import pytest

import compress_edges as ce
import compress_frames as cf
from compress_split import blocks_of
from test_compress_fse_gpu import POISON, ctx, cz, decode_three_ways, tiled  # noqa: F401  (fixtures and helpers)
from test_emu_encode_fast_split import FIELDS, GROUP, LENGTHS, SUB, three_groups
from test_emu_encode_fast import mixed_group, raw_groups

pytestmark = pytest.mark.gpu
FAST, FAST_SPLIT = 32, 128
OK, TOO_SMALL = 0, 900


def device_compress(cz, ctx, bufs, caps=None, in_shift=3, **kw):
    """Through cz_compress_batch_device with torch buffers: inputs at odd offsets, output regions of `caps` bytes (default: the
    bound) poisoned, the gaps between them checked.  Returns [(result, whole region)]."""
    import torch
    lens = [len(b) for b in bufs]
    in_off = np.cumsum([in_shift] + [n + 1 for n in lens[:-1]]).astype(np.uint64)
    host_in = np.zeros(int(in_off[-1]) + lens[-1] + 16, dtype=np.uint8)
    for o, b in zip(in_off, bufs):
        host_in[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    caps = [cz.compress_bound(n) for n in lens] if caps is None else list(caps)
    out_off = np.cumsum([5] + [c + 3 for c in caps[:-1]]).astype(np.uint64)
    total = int(out_off[-1]) + caps[-1] + 64
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(host_in).to(dev)
    d_out = torch.full((total,), POISON, dtype=torch.uint8, device=dev)
    desc = torch.from_numpy(np.stack([in_off, np.array(lens, dtype=np.uint64), out_off, np.array(caps, dtype=np.uint64)]).view(np.int64)).to(dev)
    d_res = torch.zeros(len(bufs) * 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.compress_batch_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(bufs), d_out.data_ptr(), desc[2].data_ptr(),
                              desc[3].data_ptr(), d_res.data_ptr(), **kw)
    ctx.synchronize()
    out = d_out.cpu().numpy()
    res = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)
    assert (out[:int(out_off[0])] == POISON).all()
    ends = out_off + np.array(caps, dtype=np.uint64)
    for i in range(len(bufs) - 1):                                      # the 3-byte gaps between regions
        assert (out[int(ends[i]):int(out_off[i + 1])] == POISON).all(), i
    assert (out[int(ends[-1]):] == POISON).all()
    return [(res[i], out[int(out_off[i]):int(out_off[i]) + caps[i]].tobytes()) for i in range(len(bufs))]


def same(name, got, want, cks):
    """A fast-split launch against the fast launch of the same batch and caps: fields, flags, every byte of the region (poison past
    bytes_written included)."""
    assert len(got) == len(want)
    for i, ((r, region), (q, wanted)) in enumerate(zip(got, want)):
        for k in FIELDS:
            assert int(r[k]) == int(q[k]), (name, i, k, int(r[k]), int(q[k]))
        assert int(r["flags"]) == FAST_SPLIT | cks and int(q["flags"]) == FAST | cks, (name, i, int(r["flags"]))
        assert region == wanted, f"{name}[{i}]: the output region differs from the fast level's"
        assert (np.frombuffer(region, dtype=np.uint8)[int(r["bytes_written"]):] == POISON).all(), f"{name}[{i}]: bytes past bytes_written were touched"


def frames(got):
    for i, (r, _) in enumerate(got):
        assert int(r["status"]) == OK, (i, int(r["status"]))
    return [region[:int(r["bytes_written"])] for r, region in got]


@pytest.fixture(scope="module")
def boundary_batch():
    text = ce.corpus_text(max(LENGTHS))
    return [text[:n] for n in LENGTHS] + [raw_groups(), mixed_group(), b"\x07" * 300000]


def test_flag_is_accepted_alone_and_with_the_checksum_only(cz, ctx):
    """128 and 129 in cz_compress_batch_device / _host; CZ_E_INVALID_ARG with each of 2, 4, 8, 16, 32 and 64 and in
    cz_compress_batch_dict_*; Python raises on the refused combinations.  (Fails without the feature: 128 is an unknown bit there.)"""
    import torch
    assert cz.COMPRESS_FAST_SPLIT == 128
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

    for flags in (128, 129):
        assert both(flags) == (cz.status.CZ_OK, cz.status.CZ_OK), flags
        r = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)[0]
        assert int(r["status"]) == 0 and int(r["flags"]) == flags
        dev = d_out.cpu().numpy()[:int(r["bytes_written"])].tobytes()
        assert int(h_res[0]["status"]) == 0 and int(h_res[0]["flags"]) == flags
        assert h_out[:int(h_res[0]["bytes_written"])].tobytes() == dev
        assert cf.libzstd() is None or cf.libzstd_decompress(dev, len(src)) == src
        assert dev == cz.compress(src, ctx, checksum=bool(flags & 1), fast=True)
    for bit in (2, 4, 8, 16, 32, 64):
        for flags in (128 | bit, 129 | bit):
            assert both(flags) == (cz.status.CZ_E_INVALID_ARG, cz.status.CZ_E_INVALID_ARG), flags
    p, hp = d_res.data_ptr(), h_res.ctypes.data
    for flags in (128, 129):
        assert L.cz_compress_batch_dict_device(ctx._h, p, p, p, 1, p, p, p, flags, p, p) == cz.status.CZ_E_INVALID_ARG
        assert L.cz_compress_batch_dict_host(ctx._h, hp, 8, hp, hp, 1, hp, 32, hp, hp, flags, hp, hp) == cz.status.CZ_E_INVALID_ARG
    for kw in ({"split": True}, {"fse_tables": True}, {"fast": True}, {"records": True}):
        with pytest.raises(cz.CzError):
            cz.compress(src, ctx, fast_split=True, **kw)
    with pytest.raises(cz.CzError):
        cz.compress_batch_host_dict([src], None, ctx, fast_split=True)


@pytest.mark.parametrize("checksum", (False, True))
def test_boundary_batch_equals_the_fast_level_and_decodes(cz, ctx, boundary_batch, checksum):
    got = device_compress(cz, ctx, boundary_batch, checksum=checksum, fast_split=True)
    want = device_compress(cz, ctx, boundary_batch, checksum=checksum, fast=True)
    same("boundary", got, want, int(checksum))
    fr = frames(got)
    for b, f, (r, _) in zip(boundary_batch, fr, got):
        assert int(r["bytes_read"]) == len(b) and int(r["blocks"]) == len(blocks_of(f)[1]) and len(f) <= cz.compress_bound(len(b))
    assert [len(blocks_of(f)[1]) for f in fr[len(LENGTHS):]] == [2, 4, 10]   # Raw groups are one block each
    decode_three_ways(cz, boundary_batch, fr, checksum=checksum)


def test_more_units_than_workgroups_alone_reversed_inside_and_twice(cz, ctx):
    """400 buffers of three groups each (text tiled to 300 KiB, each from its own skip): 1 200 units.  Alone, reversed, inside a
    larger batch and twice in a row the frames are identical, and they are the fast level's."""
    text = ce.corpus_text(64 << 10)
    pool = text * ((300 << 10) // len(text) + 3)
    bufs = [pool[37 * i + 1: 37 * i + 1 + (300 << 10)] for i in range(400)]
    assert len(set(bufs)) == 400 and all(len(b) == 300 << 10 for b in bufs)
    alone = device_compress(cz, ctx, bufs, fast_split=True)
    want = device_compress(cz, ctx, bufs, fast=True)
    same("alone", alone, want, 0)
    assert all(int(r["blocks"]) == 10 for r, _ in alone)
    fr = frames(alone)
    assert frames(device_compress(cz, ctx, bufs, in_shift=1, fast_split=True)) == fr      # twice in a row
    assert frames(device_compress(cz, ctx, bufs[::-1], fast_split=True))[::-1] == fr
    small = [text[:1], b"", text[:SUB + 1], three_groups()]
    inside = frames(device_compress(cz, ctx, small + bufs[:200] + small[::-1] + bufs[200:] + small, in_shift=2, fast_split=True))
    assert inside[4:204] + inside[208:408] == fr
    assert inside[:4] == inside[204:208][::-1] == inside[408:] == frames(device_compress(cz, ctx, small, fast=True))
    decode_three_ways(cz, bufs[:3] + bufs[-1:], fr[:3] + fr[-1:])


def test_one_16_mib_buffer_with_the_checksum(cz, ctx):
    big = tiled(1, 16 << 20, seed=5)[0]
    got = device_compress(cz, ctx, [big], checksum=True, fast_split=True)
    want = device_compress(cz, ctx, [big], checksum=True, fast=True)
    same("16 MiB", got, want, 1)
    (r, region), = got
    assert int(r["status"]) == OK and int(r["bytes_read"]) == len(big)
    import oracle
    assert int(r["checksum"]) == oracle.xxh64(big) & 0xFFFFFFFF
    st, out, info = oracle.decode_frame(region[:int(r["bytes_written"])], cap=len(big) + 64)
    assert st == 0 and out == big and info["has_checksum"]


@pytest.mark.parametrize("checksum", (False, True))
def test_out_cap_sweep(cz, ctx, checksum):
    """header - 1, header, the end of each group - 1 and exact, with the checksum full - 1 and full, in one batch next to frames
    that fit: every field and every byte as from the fast level at the same caps."""
    three = three_groups()
    (r, region), = device_compress(cz, ctx, [three], checksum=checksum, fast=True)
    full = int(r["bytes_written"])
    hl, blocks = blocks_of(region[:full])
    assert [b[2] for b in blocks] == [2, 1, 1, 1, 0, 2]
    ends = [blocks[4][0], blocks[5][0], blocks[5][0] + blocks[5][4]]
    caps = [hl - 1, hl] + [e - d for e in ends for d in (1, 0)] + ([full - 1, full] if checksum else [])
    bufs = [three] * len(caps) + [three[:GROUP + 7]]
    caps = caps + [cz.compress_bound(GROUP + 7)]
    got = device_compress(cz, ctx, bufs, caps=caps, checksum=checksum, fast_split=True)
    want = device_compress(cz, ctx, bufs, caps=caps, checksum=checksum, fast=True)
    same("sweep", got, want, int(checksum))
    rec = [tuple(int(r[k]) for k in ("status", "blocks", "bytes_read", "bytes_written")) for r, _ in got]
    n = len(three)
    assert rec[0] == (TOO_SMALL, 0, 0, 0)
    assert rec[1] == rec[2] == (TOO_SMALL, 0, 0, hl)
    assert rec[3] == rec[4] == (TOO_SMALL, 4, GROUP, ends[0])
    assert rec[5] == rec[6] == (TOO_SMALL, 5, 2 * GROUP, ends[1])
    if checksum:
        assert rec[7] == rec[8] == (TOO_SMALL, 6, n, ends[2]) and rec[9] == (OK, 6, n, full)
    else:
        assert rec[7] == (OK, 6, n, full)
    assert rec[-1][0] == OK and rec[-1][2] == GROUP + 7


def test_host_path_matches_device_path(cz, ctx, boundary_batch):
    for checksum in (False, True):
        got = device_compress(cz, ctx, boundary_batch, checksum=checksum, fast_split=True)
        host = cz.compress_batch_host(boundary_batch, ctx, checksum=checksum, fast_split=True)
        assert [fr for _, fr in host] == frames(got)
        for (r, _), (q, _) in zip(host, got):
            assert [int(r[k]) for k in FIELDS + ("flags",)] == [int(q[k]) for k in FIELDS + ("flags",)]
    assert cz.compress(boundary_batch[11], ctx, checksum=True, fast_split=True) == frames(got)[11]


def test_other_levels_are_unchanged_around_a_fast_split_launch(cz, ctx):
    """Frames of flags 0, 4, 16, 32 and 64 on the same context, before and after: no state leaks between the kernels."""
    some = tiled(8, 128 << 10, seed=21) + tiled(1, 700_000, seed=9) + [three_groups()]
    small = [b[:20000] for b in some]

    def others():
        return [[fr for _, fr in cz.compress_batch_host(some, ctx, **kw)] for kw in ({}, {"split": True}, {"fse_tables": True}, {"fast": True})] \
            + [[fr for _, fr in cz.compress_batch_host(small, ctx, records=True)]]

    before = others()
    mine = [fr for _, fr in cz.compress_batch_host(some, ctx, fast_split=True)]
    after = others()
    again = [fr for _, fr in cz.compress_batch_host(some, ctx, fast_split=True)]
    assert before == after and mine == again
    assert mine == before[3]                                            # the fast level's frames
    assert all(a != b for a, b in zip(mine, before[0]))
