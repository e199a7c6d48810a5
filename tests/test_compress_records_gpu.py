"""CZ_COMPRESS_RECORDS on the MI355X (cz_compress_records_kernel, cz_compress_records_dict_kernel): which flags go with it, through
the C ABI on both paths; the device's frames equal the emulator's (sha256 manifest) and, without a dictionary, the device's own
CZ_COMPRESS_FAST frames; 4 000 records with dictionaries in one launch come back through this library's decoder, the oracle and
libzstd; host path = device path; the bytes do not depend on the batch; and the other levels write what they wrote before and
after a records launch.  Run with `pytest -m gpu`."""
import hashlib
import json
import os

import numpy as np
import pytest

import compress_edges as ce
import compress_frames as cf
import dict_frames as dfr
import dict_records as dr
import records_edges as rede
from compress_split import blocks_of
from test_compress_dict_gpu import NO_DICT, POISON, ctx, cz, dicts  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
R, MAXREC = 64, 32 << 10
MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compress_records", "manifest.json")
LENGTHS = (0, 1, 15, 16, 17, 255, 256, 6724, 6725, MAXREC - 1, MAXREC)


def device_compress(cz, ctx, bufs, idx="plain", caps=None, checksum=False, dict_id=True, in_shift=0, records=True, fast=False):
    """Through cz_compress_batch_device (idx "plain") or cz_compress_batch_dict_device (idx a list, or None for no index) with torch
    buffers: inputs at odd offsets (moved by in_shift), output regions poisoned, the gaps between the regions checked, the result
    records poisoned with 0xA5.  Returns [(result, whole region)]."""
    import torch
    lens = [len(b) for b in bufs]
    in_off = np.cumsum([3 + in_shift] + [n + 1 for n in lens[:-1]]).astype(np.uint64)
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
    d_res = torch.full((len(bufs) * 32,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    if isinstance(idx, str):
        ctx.compress_batch_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(bufs), d_out.data_ptr(), desc[2].data_ptr(),
                                  desc[3].data_ptr(), d_res.data_ptr(), checksum=checksum, records=records, fast=fast)
    else:
        d_idx = torch.from_numpy(np.array(idx, dtype=np.uint32).view(np.int32)).to(dev) if idx is not None else None
        ctx.compress_batch_dict_device(d_in.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), len(bufs), d_out.data_ptr(), desc[2].data_ptr(),
                                       desc[3].data_ptr(), d_idx.data_ptr() if d_idx is not None else 0, d_res.data_ptr(), checksum=checksum,
                                       dict_id=dict_id, records=records)
    ctx.synchronize()
    out = d_out.cpu().numpy()
    res = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)
    assert (out[:int(out_off[0])] == POISON).all()
    ends = out_off + np.array(caps, dtype=np.uint64)
    gaps = np.ones(total, dtype=bool)
    for o, e in zip(out_off, ends):
        gaps[int(o):int(e)] = False
    assert (out[gaps] == POISON).all(), "a byte between the regions was written"
    return [(res[i], out[int(out_off[i]):int(out_off[i]) + caps[i]].tobytes()) for i in range(len(bufs))]


def frames_of(cz, bufs, got, flags):
    """The frames of `got`, each checked: status 0, the flags, one block, the bound, poison past bytes_written."""
    frames = []
    for i, (b, (r, region)) in enumerate(zip(bufs, got)):
        n = int(r["bytes_written"])
        assert int(r["status"]) == 0 and int(r["flags"]) == flags, (i, r)
        assert n <= cz.compress_bound(len(b)) and int(r["bytes_read"]) == len(b) and int(r["blocks"]) == 1, (i, r)
        assert (np.frombuffer(region, dtype=np.uint8)[n:] == POISON).all(), f"frame {i}: bytes past bytes_written were touched"
        assert len(blocks_of(region[:n])[1]) == 1, i
        frames.append(region[:n])
    return frames


def test_flag_acceptance_and_refusal(cz, ctx, dicts):
    """64 and 65 in cz_compress_batch_device / _host; 64, 65, 66 and 67 in cz_compress_batch_dict_device / _host; CZ_E_INVALID_ARG
    with SPLIT, FSE_TABLES, FAST and bit 8.  (Fails without the feature: bit 64 is an unknown bit there.)"""
    import torch
    assert cz.COMPRESS_RECORDS == 64 and cz.compress_record_max() == 32768 == int(cz.lib().cz_compress_record_max())
    L = cz.lib()
    src = dr.records(1, seed=3)[0][1]
    cap = cz.compress_bound(len(src))
    d_in = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).to("cuda:0")
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    desc = torch.tensor([0, len(src), 0, cap], dtype=torch.int64, device="cuda:0")
    d_idx = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    d_res = torch.zeros(32, dtype=torch.uint8, device="cuda:0")
    h_in, h_out = np.frombuffer(src, dtype=np.uint8).copy(), np.zeros(cap, dtype=np.uint8)
    h_desc, h_res, h_idx = np.array([0, len(src), 0, cap], dtype=np.uint64), np.zeros(1, dtype=cz.COMPRESS_RESULT_DTYPE), np.zeros(1, dtype=np.uint32)

    def both(flags, with_dict):
        if with_dict:
            st_d = L.cz_compress_batch_dict_device(ctx._h, d_in.data_ptr(), desc[0:].data_ptr(), desc[1:].data_ptr(), 1, d_out.data_ptr(),
                                                   desc[2:].data_ptr(), desc[3:].data_ptr(), flags, d_idx.data_ptr(), d_res.data_ptr())
            ctx.synchronize()
            st_h = L.cz_compress_batch_dict_host(ctx._h, h_in.ctypes.data, h_in.size, h_desc[0:].ctypes.data, h_desc[1:].ctypes.data, 1,
                                                 h_out.ctypes.data, h_out.size, h_desc[2:].ctypes.data, h_desc[3:].ctypes.data, flags,
                                                 h_idx.ctypes.data, h_res.ctypes.data)
        else:
            st_d = L.cz_compress_batch_device(ctx._h, d_in.data_ptr(), desc[0:].data_ptr(), desc[1:].data_ptr(), 1, d_out.data_ptr(),
                                              desc[2:].data_ptr(), desc[3:].data_ptr(), flags, d_res.data_ptr())
            ctx.synchronize()
            st_h = L.cz_compress_batch_host(ctx._h, h_in.ctypes.data, h_in.size, h_desc[0:].ctypes.data, h_desc[1:].ctypes.data, 1,
                                            h_out.ctypes.data, h_out.size, h_desc[2:].ctypes.data, h_desc[3:].ctypes.data, flags, h_res.ctypes.data)
        return st_d, st_h

    for with_dict, ok in ((False, (64, 65)), (True, (64, 65, 66, 67))):
        for flags in ok:
            assert both(flags, with_dict) == (cz.status.CZ_OK, cz.status.CZ_OK), (with_dict, flags)
            r = d_res.cpu().numpy().view(cz.COMPRESS_RESULT_DTYPE)[0]
            assert int(r["status"]) == 0 and int(r["flags"]) == flags & ~2 and int(r["blocks"]) == 1
            dev = d_out.cpu().numpy()[:int(r["bytes_written"])].tobytes()
            assert int(h_res[0]["status"]) == 0 and int(h_res[0]["flags"]) == flags & ~2
            assert h_out[:int(h_res[0]["bytes_written"])].tobytes() == dev
            if dr.libzstd():
                assert dr.zstd_decompress_dict(dev, len(src), dr.dictionaries()[0] if with_dict else None) == src
        for flags in (64 | 4, 64 | 16, 64 | 32, 64 | 8):
            assert both(flags, with_dict) == (cz.status.CZ_E_INVALID_ARG, cz.status.CZ_E_INVALID_ARG), (with_dict, flags)
    assert both(64 | 2, False) == (cz.status.CZ_E_INVALID_ARG, cz.status.CZ_E_INVALID_ARG)      # NO_DICT_ID's bit, without dictionaries
    for flags in (32, 33):                                                                   # what was refused stays refused
        assert both(flags, True) == (cz.status.CZ_E_INVALID_ARG, cz.status.CZ_E_INVALID_ARG), flags
    for kw in ({"split": True}, {"fse_tables": True}, {"fast": True}):
        with pytest.raises(cz.CzError):
            cz.compress(src, ctx, records=True, **kw)
    assert cz.compress(src, ctx, records=True, checksum=True) == cz.compress_batch_host([src], ctx, records=True, checksum=True)[0][1]


def test_device_frames_equal_the_emulators(cz, ctx, dicts):
    m = json.load(open(MANIFEST))
    bufs, idx = rede.manifest_batch()
    assert len(bufs) == m["n"] and sorted(m["flags"]) == ["64", "65", "66", "67"]
    for flags, want in m["flags"].items():
        flags = int(flags)
        got = device_compress(cz, ctx, bufs, idx, checksum=bool(flags & 1), dict_id=not flags & 2)
        frames = frames_of(cz, bufs, got, flags & ~2)
        bad = [i for i, (f, w) in enumerate(zip(frames, want)) if hashlib.sha256(f).hexdigest() != w]
        assert not bad, (flags, bad)


def test_without_a_dictionary_the_frames_are_the_fast_levels(cz, ctx, dicts):
    text = ce.corpus_text(MAXREC + 1)
    bufs = [text[:n] for n in LENGTHS] + [b for _, b in cf.corpus_originals(max_len=MAXREC)] + \
           [b for _, b in sorted(cf.special_inputs().items()) if len(b) <= MAXREC]
    for checksum in (False, True):
        ck = 1 if checksum else 0
        rec = device_compress(cz, ctx, bufs, checksum=checksum)
        fast = device_compress(cz, ctx, bufs, checksum=checksum, records=False, fast=True)
        assert frames_of(cz, bufs, rec, R | ck) == [region[:int(r["bytes_written"])] for r, region in fast]
        for (r, _), (r2, _) in zip(rec, fast):
            assert all(int(r[k]) == int(r2[k]) for k in ("status", "blocks", "bytes_read", "bytes_written", "checksum")) and int(r2["flags"]) == 32 | ck
        nod = device_compress(cz, ctx, bufs, [NO_DICT] * len(bufs), checksum=checksum)      # the dict kernel without a dictionary
        assert [x[1] for x in nod] == [x[1] for x in rec]
    # one byte too many fails alone, on both kernels, and so does an output one byte too small
    need = int(rec[-1][0]["bytes_written"])
    for idx in ("plain", [0, 0, NO_DICT]):
        three = [bufs[5], text, bufs[-1]]
        got = device_compress(cz, ctx, three, idx, caps=[cz.compress_bound(len(three[0])), cz.compress_bound(len(text)), need - 1], checksum=True)
        assert int(got[0][0]["status"]) == 0
        r, region = got[1]
        assert (int(r["status"]), int(r["blocks"]), int(r["bytes_read"]), int(r["bytes_written"]), int(r["flags"])) == (901, 0, 0, 0, 65)
        assert set(region) == {POISON}
        r, region = got[2]
        w = int(r["bytes_written"])
        assert int(r["status"]) == 900 and w == need - 4 and region[:w] == rec[-1][1][:w] and set(region[w:]) <= {POISON}


def test_the_loop_closes(cz, ctx, dicts):
    """4 000 records, more than the device has waves in flight: every wave takes several."""
    import oracle
    recs = dr.records(1000, seed=21)
    raw = dr.dictionaries()
    bufs, idx = [b for _, b in recs], [j for j, _ in recs]
    assert len(bufs) == 4000
    got = device_compress(cz, ctx, bufs, idx, checksum=True)
    frames = frames_of(cz, bufs, got, 65)                               # every status 0, every record written (no 0xA5 left)
    try:
        ctx.set_dictionaries(dicts)
        back = cz.decode_batch_host(frames, [len(b) + 64 for b in bufs], ctx)
    finally:
        ctx.set_dictionaries([])
    for i, ((r, out), b) in enumerate(zip(back, bufs)):
        assert int(r["status"]) == 0 and out == b, i
    ods = [oracle.Dictionary(d) for d in raw]
    for i in range(0, 4000, 20):
        st, out = oracle.decode_frame_with_dict(frames[i], ods[idx[i]], cap=len(bufs[i]) + 64)
        assert st == 0 and out == bufs[i], i
        if dr.libzstd():
            assert dr.zstd_decompress_dict(frames[i], len(bufs[i]), raw[idx[i]]) == bufs[i], i
    ids = [int(d.info["id"]) for d in ods]
    assert all(dfr.header_id(f)[1] == ids[j] for f, j in zip(frames[:64], idx[:64]))
    total, old = sum(map(len, frames)), sum(len(f) for _, f in cz.compress_batch_host_dict(bufs, idx, ctx, checksum=True))
    print(f"4000 records: {sum(map(len, bufs))} -> {total} bytes at the records level, {old} from the dictionary compressor")


def test_host_path_equals_device_path_and_determinism(cz, ctx, dicts):
    recs = dr.records(50, seed=4)
    bufs, idx = [b for _, b in recs], [j for j, _ in recs]
    dev = frames_of(cz, bufs, device_compress(cz, ctx, bufs, idx), R)
    host = cz.compress_batch_host_dict(bufs, idx, ctx, records=True)
    assert [f for _, f in host] == dev and all(int(r["flags"]) == R for r, _ in host)
    assert frames_of(cz, bufs, device_compress(cz, ctx, bufs, idx, in_shift=1), R) == dev           # again
    order = list(reversed(range(len(bufs))))[::2]                       # another order, another composition
    extra = [b"padding " * 1000, bytes(range(256)) * 40]
    mixed = device_compress(cz, ctx, extra + [bufs[i] for i in order], [NO_DICT, 2] + [idx[i] for i in order])
    assert [region[:int(r["bytes_written"])] for r, region in mixed[2:]] == [dev[i] for i in order]
    one = cz.Context(0)                                                 # NULL index with one dictionary set: every frame uses it
    try:
        d = cz.Dictionary(one, dr.dictionaries()[0])
        one.set_compress_dictionaries([d])
        users = [b for j, b in recs if j == 0]
        want = [dev[i] for i, (j, _) in enumerate(recs) if j == 0]
        assert [f for _, f in cz.compress_batch_host_dict(users, None, one, records=True)] == want
        assert frames_of(cz, users, device_compress(cz, one, users, None), R) == want
    finally:
        one.close()
    plain = cz.compress_batch_host(bufs, ctx, records=True, checksum=True)                          # the plain calls, host = device
    assert [f for _, f in plain] == frames_of(cz, bufs, device_compress(cz, ctx, bufs, checksum=True), 65)


def test_other_levels_are_unchanged_around_a_records_launch(cz, ctx, dicts):
    """No state leaks between the kernels."""
    recs = dr.records(16, seed=5)
    bufs, idx = [b for _, b in recs] + [ce.corpus_text(20000)], [j for j, _ in recs] + [1]

    def others():
        return ([f for _, f in cz.compress_batch_host(bufs, ctx)], [f for _, f in cz.compress_batch_host(bufs, ctx, fse_tables=True)],
                [f for _, f in cz.compress_batch_host(bufs, ctx, fast=True)], [f for _, f in cz.compress_batch_host_dict(bufs, idx, ctx)])
    before = others()
    rec = [f for _, f in cz.compress_batch_host_dict(bufs, idx, ctx, records=True)]
    rec_plain = [f for _, f in cz.compress_batch_host(bufs, ctx, records=True)]
    after = others()
    assert before == after
    assert rec == [f for _, f in cz.compress_batch_host_dict(bufs, idx, ctx, records=True)]
    assert rec_plain == before[2] and rec != before[3]
