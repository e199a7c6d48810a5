"""Seekable streams on the CPU (cz_seekable_bound, cz_seekable_pack_host, cz_seekable_open_host; csrc/czstd_seekable_host.h) against
the independent model of the format in seekable_model.py: packing n = 0, 1, 2 and 300 libzstd frames with and without checksums,
opening every kind of range at three alignments, each of the six table defects by its number, and the packed stream under
cz_stream_split and libzstd.  The same streams then go through the header alone in a stand-alone program under ASan + UBSan
(tests/emu/seekable_host_main.cpp), from exact-size heap blocks.  No GPU needed."""
import struct

import numpy as np
import pytest

import cairo_zstd_amd as cz
import compress_frames as cf
import oracle
import seekable_model as model
import seekable_runner as sk

NS = (0, 1, 2, 300)
BIG = (7, 150, 299)                                                      # the 200 KiB contents of the 300-frame batch
RANGES = ("all", "empty_at_end", "last", "3_5")


@pytest.fixture(scope="module")
def batches():
    """n -> (contents, frames, checksums)"""
    out = {}
    for n in NS:
        data = sk.contents(n, BIG if n == 300 else ())
        out[n] = (data, [sk.zstd_frame(d, checksum=bool(i & 1)) for i, d in enumerate(data)], [oracle.xxh64(d) & 0xFFFFFFFF for d in data])
    return out


def the_range(name, n):
    """(first, count); None for the last frame of no frames"""
    return {"all": (0, n), "empty_at_end": (n, 0), "last": (n - 1, 1) if n else None, "3_5": (3, 5)}[name]


def test_the_symbols_and_the_status_exist():
    """Fails without the feature."""
    assert cz.status.CZ_E_SEEK_TABLE == 909 == model.SEEK_TABLE and cz.SEEKABLE_CHECKSUMS == 1
    assert cz.SEEKABLE_INFO_DTYPE.itemsize == 56 and cz.SEEKABLE_INFO_DTYPE == sk.INFO_DTYPE
    L = cz.lib()
    for name in ("cz_seekable_bound", "cz_seekable_pack_device", "cz_seekable_open_device", "cz_seekable_pack_host", "cz_seekable_open_host"):
        assert hasattr(L, name), name
    for fb, n in ((0, 0), (1, 1), (12345, 300), (1 << 40, 0x8000000)):
        assert cz.seekable_bound(fb, n) == model.bound(fb, n) and cz.seekable_bound(fb, n, True) == model.bound(fb, n, True)
    assert cz.seekable_bound(0, 0) == 17


@pytest.mark.parametrize("cks", (False, True))
@pytest.mark.parametrize("n", NS)
def test_pack_equals_the_model(batches, n, cks):
    data, frames, sums = batches[n]
    want = model.build(frames, [len(d) for d in data], sums if cks else None)
    got = cz.pack_seekable(frames, [len(d) for d in data], sums if cks else None)
    assert got == want and len(got) == cz.seekable_bound(sum(len(f) for f in frames), n, cks)
    if n == 0:
        assert len(got) == 17 and got == struct.pack("<IIIBI", 0x184D2A5E, 9, 0, 0x80 if cks else 0, 0x8F92EAB1)


@pytest.mark.parametrize("align", (1, 16, 256))
@pytest.mark.parametrize("cks", (False, True))
def test_open_equals_the_model(batches, cks, align):
    for n in NS:
        data, frames, sums = batches[n]
        stream = model.build(frames, [len(d) for d in data], sums if cks else None)
        for name in RANGES:
            if the_range(name, n) is None:
                continue
            first, count = the_range(name, n)
            st, *want, need = model.open_range(stream, first, count, align)
            info, *got = cz.open_seekable(stream, first, count, align)
            assert int(info["status"]) == st, (n, name)
            if st:
                assert st == model.INVALID_ARG and first + count > n and all(g.size == 0 for g in got)
                continue
            assert [g.tolist() for g in got] == want, (n, name)
            assert int(info["detail"]) == need
            for k, v in model.info_of(stream).items():
                assert int(info[k]) == v, (n, name, k)
            if name == "all":
                assert [g.tolist() for g in cz.open_seekable(stream, 0, None, align)[1:]] == want
        assert int(cz.open_seekable(stream, n + 1, 0, align)[0]["status"]) == model.INVALID_ARG
        assert int(cz.open_seekable(stream, n + 1, None, align)[0]["status"]) == model.INVALID_ARG
        assert int(cz.open_seekable(stream, 0, n + 1, align)[0]["status"]) == model.INVALID_ARG
    # alignment really pads: the second frame of the range starts at the first one's size rounded up
    data, frames, sums = batches[300]
    info, in_off, in_len, out_off, out_cap, _ = cz.open_seekable(model.build(frames, [len(d) for d in data]), 3, 5, align)
    assert out_off.tolist() == np.concatenate([[0], np.cumsum(-(-out_cap[:-1].astype(np.int64) // align) * align)]).tolist()
    assert out_cap.tolist() == [len(d) for d in data[3:8]] and in_len.tolist() == [len(f) for f in frames[3:8]]


def test_bad_alignments_are_refused(batches):
    data, frames, _ = batches[2]
    stream = model.build(frames, [len(d) for d in data])
    for align in (0, 3, 24, 8192, 4097):
        assert int(cz.open_seekable(stream, 0, None, align)[0]["status"]) == model.INVALID_ARG, align
    assert int(cz.open_seekable(stream, 0, None, 4096)[0]["status"]) == 0


@pytest.mark.parametrize("cks", (False, True))
def test_each_of_the_six_reasons_by_its_number(batches, cks):
    data, frames, sums = batches[300]
    stream = model.build(frames, [len(d) for d in data], sums if cks else None)
    bad = model.damaged(stream)
    assert sorted(bad) == list(model.REASONS)
    for reason, s in list(bad.items()) + model.damaged_more(stream):
        info, *arrays = cz.open_seekable(s, 0, None, 1)
        assert (int(info["status"]), int(info["reason"])) == (cz.status.CZ_E_SEEK_TABLE, reason), reason
        assert all(a.size == 0 for a in arrays)
        for k, v in model.info_of(s).items():
            assert int(info[k]) == v, (reason, k)
    assert int(cz.open_seekable(b"", 0, None, 1)[0]["reason"]) == 1


def test_unused_descriptor_bits_are_ignored(batches):
    data, frames, sums = batches[2]
    for cks in (None, sums):
        good = model.build(frames, [len(d) for d in data], cks)
        for bits in (1, 2, 3):
            s = bytearray(good)
            s[-5] |= bits
            assert model.parse(bytes(s))[0] == 0
            a, b = cz.open_seekable(bytes(s)), cz.open_seekable(good)
            assert int(a[0]["status"]) == 0 and [x.tolist() for x in a[1:]] == [x.tolist() for x in b[1:]]


@pytest.mark.parametrize("cks", (False, True))
def test_every_decoder_still_reads_the_stream(batches, cks):
    """cz_stream_split: n frame entries and one skippable entry with the seek table's magic; libzstd decodes frame by frame at the
    model's offsets, and the whole stream in one call."""
    data, frames, sums = batches[300]
    stream = cz.pack_seekable(frames, [len(d) for d in data], sums if cks else None)
    st, ents, consumed = cz.stream_split(stream)
    assert st == 0 and consumed == len(stream) and len(ents) == 301
    assert (ents["kind"][:300] == cz.STREAM_FRAME).all() and int(ents["kind"][300]) == cz.STREAM_SKIPPABLE and int(ents["magic"][300]) == 0x184D2A5E
    _, in_off, in_len, _, out_cap, got_sums, _ = model.open_range(stream)
    assert ents["offset"][:300].tolist() == in_off and ents["length"][:300].tolist() == in_len
    assert got_sums == (sums if cks else [0] * 300)
    assert cf.libzstd() is not None
    for i in (0, 1, 2, 7, 40, 41, 150, 298, 299):
        assert cf.libzstd_decompress(stream[in_off[i]:in_off[i] + in_len[i]], out_cap[i]) == data[i], i
    assert cf.libzstd_decompress(stream, sum(out_cap)) == b"".join(data)


def test_pack_refuses_what_it_must(batches):
    """A failed record, a size of 2^32, a record without the checksum under SEEKABLE_CHECKSUMS: CZ_E_INVALID_ARG with the lowest index;
    a cap one short: CZ_E_OUTPUT_TOO_SMALL with the need; unknown flag bits; nothing written in any of these."""
    data, frames, sums = batches[2]
    L = cz.lib()
    base = np.frombuffer(b"".join(frames) + b"\0", dtype=np.uint8)
    off = np.array([0, len(frames[0])], dtype=np.uint64)
    need = model.bound(len(base) - 1, 2, True)

    def pack(res, flags, cap):
        out = np.full(need + 8, 0xEE, dtype=np.uint8)
        info = np.zeros(1, dtype=cz.SEEKABLE_INFO_DTYPE)
        st = L.cz_seekable_pack_host(base.ctypes.data, off.ctypes.data, res.ctypes.data, 2, out.ctypes.data, cap, flags, info.ctypes.data)
        assert st == int(info[0]["status"])
        return st, info[0], out

    good = sk.records([len(f) for f in frames], [len(d) for d in data], sums)
    st, info, out = pack(good, 1, need)
    assert st == 0 and int(info["stream_bytes"]) == need and out[:need].tobytes() == model.build(frames, [len(d) for d in data], sums)
    assert (out[need:] == 0xEE).all()
    st, info, out = pack(good, 1, need - 1)
    assert st == model.TOO_SMALL and int(info["stream_bytes"]) == need and (out == 0xEE).all()
    for field, value in (("status", 900), ("bytes_written", 1 << 32), ("bytes_read", 1 << 32), ("flags", 64)):
        for i in (0, 1):
            res = good.copy()
            res[field][i] = value
            st, info, out = pack(res, 1, need)
            assert st == model.INVALID_ARG and int(info["detail"]) == i and (out == 0xEE).all(), (field, i)
    res = good.copy()
    res["flags"] = 0
    assert pack(res, 0, need)[0] == 0                                    # without the flag the records need no checksum
    for flags in (2, 3, 4, 0x80000000):
        st, info, out = pack(good, flags, need)
        assert st == model.INVALID_ARG and (out == 0xEE).all()


def host_cases(batches):
    """The good and the damaged streams for the stand-alone program: ([case bytes], [what to expect])."""
    cases, want = [], []
    for n in NS:
        data, frames, sums = batches[n]
        sizes = [len(d) for d in data]
        for cks in (None, sums):
            stream = model.build(frames, sizes, cks)
            cases.append(sk.pack_case(frames, sk.records([len(f) for f in frames], sizes, cks), flags=int(cks is not None), residue=n % 16))
            want.append(("pack", stream, n % 16))
            for name in RANGES:
                if the_range(name, n) is None:
                    continue
                first, count = the_range(name, n)
                st, *arrays, need = model.open_range(stream, first, count, 16)
                cases.append(sk.open_case(stream, first, count, 16, k=len(arrays[0]), residue=1 + n % 5))
                want.append(("open", st, arrays, need, model.info_of(stream)))
            cases.append(sk.open_case(stream, 0, sk.ALL, 1, k=0, arrays=False))
            want.append(("open", 0, [[]] * 5, model.open_range(stream)[-1], model.info_of(stream)))
    data, frames, sums = batches[300]
    stream = model.build(frames, [len(d) for d in data], sums)
    for reason, s in list(model.damaged(stream).items()) + model.damaged_more(stream):
        cases.append(sk.open_case(s, 0, sk.ALL, 1, k=300 if reason != 1 else 0))
        want.append(("bad", reason, model.info_of(s)))
    return cases, want


def test_the_header_alone_under_the_sanitizers(batches):
    """czstd_seekable_host.h compiled by g++ with -fsanitize=address,undefined into a program of its own: the same answers, from
    exact-size heap blocks, and poison wherever nothing may be written."""
    cases, want = host_cases(batches)
    got = sk.run(sk.HOST, cases)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        ret, info = g[0], g[1]
        assert ret == int(info["status"]), i
        if w[0] == "pack":
            _, stream, residue = w
            assert ret == 0 and g[2] == b"\xEE" * residue + stream, i
            assert int(info["stream_bytes"]) == len(stream) and int(info["frames_bytes"]) == model.info_of(stream)["frames_bytes"]
        elif w[0] == "open":
            _, st, arrays, need, inf = w
            assert ret == st, i
            for k, v in inf.items():
                if k != "status":
                    assert int(info[k]) == v, (i, k)
            if st == 0:
                assert [a.tolist() for a in g[2:]] == [list(a) for a in arrays] and int(info["detail"]) == need, i
            else:
                assert all(set(a.tobytes()) <= {0xA5} for a in g[2:]), i
        else:
            _, reason, inf = w
            assert (ret, int(info["reason"])) == (model.SEEK_TABLE, reason), i
            assert all(int(info[k]) == v for k, v in inf.items())
            assert all(set(a.tobytes()) <= {0xA5} for a in g[2:]), f"case {i}: an array was written on a table error"
