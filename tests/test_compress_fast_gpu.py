"""CZ_COMPRESS_FAST on the MI355X (cz_compress_frames_fast_kernel): the flag is accepted alone and with the checksum and refused with
CZ_COMPRESS_SPLIT, CZ_COMPRESS_FSE_TABLES, unknown bits and dictionaries; its frames decode under the oracle, libzstd and this
library's decoder (single launch and the pre-pass pipeline with checksums verified), stay within the bound and keep the format's
rules (blocks of at most 32 KiB that stand alone, Raw groups); host path = device path; the bytes do not depend on the batch; and the
other compress kernels write what they wrote before and after a fast launch.  Run with `pytest -m gpu`."""
import numpy as np
import pytest

import compress_edges as ce
import compress_frames as cf
import compress_fse as fx
from compress_split import blocks_of
from test_compress_fse_gpu import POISON, batch, ctx, cz, decode_three_ways, tiled  # noqa: F401  (fixtures and helpers)
from test_emu_encode_fast import LENGTHS, SUB, mixed_group, raw_groups, structure

pytestmark = pytest.mark.gpu
FAST = 32


def device_compress(cz, ctx, bufs, in_shift=3, checksum=False):
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
                              desc[3].data_ptr(), d_res.data_ptr(), checksum=checksum, fast=True)
    ctx.synchronize()
    out = d_out.cpu().numpy()
    res = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)
    assert (out[:int(out_off[0])] == POISON).all()
    ends = out_off + np.array(caps, dtype=np.uint64)
    for i in range(len(bufs) - 1):                                      # the 3-byte gaps between regions
        assert (out[int(ends[i]):int(out_off[i + 1])] == POISON).all(), i
    assert (out[int(ends[-1]):] == POISON).all()
    return [(res[i], out[int(out_off[i]):int(out_off[i]) + caps[i]].tobytes()) for i in range(len(bufs))]


def frames_of(cz, bufs, got, flags=FAST):
    """The frames of `got`, each checked: status, bound, poison past bytes_written, the record (blocks from the frame's own block
    list) and its flags."""
    frames = []
    for i, (b, (r, region)) in enumerate(zip(bufs, got)):
        n = int(r["bytes_written"])
        assert int(r["status"]) == 0, (i, int(r["status"]))
        assert n <= cz.compress_bound(len(b))
        assert (np.frombuffer(region, dtype=np.uint8)[n:] == POISON).all(), f"frame {i}: bytes past bytes_written were touched"
        assert int(r["bytes_read"]) == len(b) and int(r["blocks"]) == len(blocks_of(region[:n])[1]), i
        assert int(r["flags"]) == flags, (i, int(r["flags"]))
        frames.append(region[:n])
    return frames


@pytest.fixture(scope="module")
def boundary_batch():
    text = ce.corpus_text(max(LENGTHS))
    return [text[:n] for n in LENGTHS] + [raw_groups(), mixed_group(), b"\x07" * 300000]


def test_flag_is_accepted_alone_and_with_the_checksum_only(cz, ctx):
    """32 and 33 in cz_compress_batch_device / _host; CZ_E_INVALID_ARG with SPLIT, FSE_TABLES, NO_DICT_ID's bit, bit 8 and in
    cz_compress_batch_dict_*.  (Fails without the feature: bit 32 is an unknown bit there.)"""
    import torch
    assert cz.COMPRESS_FAST == 32
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

    for flags in (32, 33):
        assert both(flags) == (cz.status.CZ_OK, cz.status.CZ_OK), flags
        r = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)[0]
        assert int(r["status"]) == 0 and int(r["flags"]) == flags
        dev = d_out.cpu().numpy()[:int(r["bytes_written"])].tobytes()
        assert int(h_res[0]["status"]) == 0 and int(h_res[0]["flags"]) == flags
        assert h_out[:int(h_res[0]["bytes_written"])].tobytes() == dev
        assert cf.libzstd() is None or cf.libzstd_decompress(dev, len(src)) == src
    for flags in (32 | 4, 32 | 16, 32 | 2, 32 | 8):
        assert both(flags) == (cz.status.CZ_E_INVALID_ARG, cz.status.CZ_E_INVALID_ARG), flags
    p, hp = d_res.data_ptr(), h_res.ctypes.data
    for flags in (32, 33):
        assert L.cz_compress_batch_dict_device(ctx._h, p, p, p, 1, p, p, p, flags, p, p) == cz.status.CZ_E_INVALID_ARG
        assert L.cz_compress_batch_dict_host(ctx._h, hp, 8, hp, hp, 1, hp, 32, hp, hp, flags, hp, hp) == cz.status.CZ_E_INVALID_ARG
    for kw in ({"split": True}, {"fse_tables": True}):
        with pytest.raises(cz.CzError):
            cz.compress(src, ctx, fast=True, **kw)


def test_corpus_three_decoders_and_size(cz, ctx):
    names, bufs = zip(*cf.corpus_originals())
    assert len(bufs) == 69
    got = cz.compress_batch_host(list(bufs), ctx, fast=True)
    frames = [fr for _, fr in got]
    for name, b, (r, fr) in zip(names, bufs, got):
        assert int(r["status"]) == 0 and int(r["bytes_read"]) == len(b) and int(r["flags"]) == FAST, name
        assert len(fr) <= cz.compress_bound(len(b))
    decode_three_ways(cz, bufs, frames)
    total = sum(map(len, frames))
    print(f"corpus: {sum(map(len, bufs))} -> {total} bytes at the fast level")
    assert total < sum(map(len, bufs))
    with_sum = cz.compress_batch_host(list(bufs[::3]), ctx, checksum=True, fast=True)
    assert all(int(r["flags"]) == 33 for r, _ in with_sum)
    decode_three_ways(cz, bufs[::3], [fr for _, fr in with_sum], checksum=True)


def test_tiled_batch_keeps_poison_and_its_structure(cz, ctx, batch):
    on = frames_of(cz, batch, device_compress(cz, ctx, batch))
    decode_three_ways(cz, batch, on)
    print(f"64 x 128 KiB: ratio {sum(map(len, batch)) / sum(map(len, on)):.3f} at the fast level")
    rev = frames_of(cz, batch[::-1], device_compress(cz, ctx, batch[::-1], in_shift=1))[::-1]
    assert rev == on                                                    # the bytes do not depend on the batch
    for i in range(4):
        structure(f"tiled[{i}]", batch[i], on[i])


def test_boundaries_and_raw_groups(cz, ctx, boundary_batch):
    fr = frames_of(cz, boundary_batch, device_compress(cz, ctx, boundary_batch))
    decode_three_ways(cz, boundary_batch, fr)
    for n, f in zip(LENGTHS, fr):
        assert len(blocks_of(f)[1]) == max(1, -(-n // SUB)), n
    assert fr[0] == bytes.fromhex("28b52ffd2000010000")
    raw, mixed, rle = (blocks_of(f) for f in fr[len(LENGTHS):])
    assert [(b[2], b[3]) for b in raw[1]] == [(0, 128 << 10), (0, 40000)] and len(fr[len(LENGTHS)]) == raw[0] + 6 + (128 << 10) + 40000
    assert [b[2] for b in mixed[1]] == [0, 0, 0, 2]
    assert len(rle[1]) == 10 and {b[2] for b in rle[1]} == {1}
    for name, b, f in zip(("128K+1", "160K+5", "mixed"), (boundary_batch[9], boundary_batch[10], boundary_batch[12]), (fr[9], fr[10], fr[12])):
        structure(name, b, f)


def test_host_path_matches_device_path(cz, ctx, boundary_batch):
    for checksum in (False, True):
        got = device_compress(cz, ctx, boundary_batch, checksum=checksum)
        dev = frames_of(cz, boundary_batch, got, FAST | (1 if checksum else 0))
        host = cz.compress_batch_host(boundary_batch, ctx, checksum=checksum, fast=True)
        assert [fr for _, fr in host] == dev
        assert [(int(r["flags"]), int(r["blocks"])) for r, _ in host] == [(int(r["flags"]), int(r["blocks"])) for r, _ in got]
    assert cz.compress(boundary_batch[10], ctx, checksum=True, fast=True) == dev[10]


def test_other_levels_are_unchanged_around_a_fast_launch(cz, ctx, batch):
    """No state leaks between the kernels."""
    some = batch[:16]
    before = [fr for _, fr in cz.compress_batch_host(some, ctx)]
    before_fse = [fr for _, fr in cz.compress_batch_host(some, ctx, fse_tables=True)]
    fast = [fr for _, fr in cz.compress_batch_host(some, ctx, fast=True)]
    after = [fr for _, fr in cz.compress_batch_host(some, ctx)]
    after_fse = [fr for _, fr in cz.compress_batch_host(some, ctx, fse_tables=True)]
    again = [fr for _, fr in cz.compress_batch_host(some, ctx, fast=True)]
    assert before == after and before_fse == after_fse and fast == again
    assert all(a != b for a, b in zip(fast, before))
    assert all(m["ll"] == m["of"] == m["ml"] == fx.PREDEFINED for fr in fast[:4] for m in fx.modes(fr))
