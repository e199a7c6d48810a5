"""The seekable-stream kernels (cz_seekable_plan_kernel, cz_seekable_gather_kernel, cz_seekable_open_kernel; the unmodified
czstd_seekable.hip) on the CPU SIMT emulator under ASan + UBSan (tests/emu/emu_seekable.cpp).  Every frame, the plan, the stream and
the arrays sit in exact-size heap blocks, the frames at every address residue; the stream starts as 0xEE and the arrays as 0xA5.
What comes out is compared with the model of the format (seekable_model.py) and, byte for byte and field for field, with
cz_seekable_pack_host / cz_seekable_open_host run on the same case file (tests/emu/seekable_host_main.cpp).  No GPU needed."""
import numpy as np
import pytest

import seekable_model as model
import seekable_runner as sk

pytestmark = pytest.mark.xdist_group(name="emu_seekable")
TILE = 8192                                                              # the gather's tile (checked against what the binary reports)
COUNTS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)   # around a thread's share, a wave, a workgroup, a scan tile
HUGE = 0xFFE00000


def blobs(lengths, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lengths]


class PackCase:
    """The frames in their slots, their records, and what a pack of them must give: expect None (it goes well: the model's stream)
    or (status, detail, stream_bytes)."""

    def __init__(self, frames, cks=False, residue=0, cap=None, spoil=None, expect=None, recs=None):
        self.frames, self.flags, self.residue, self.expect = frames, int(cks), residue, expect
        self.sizes = [3 * len(f) + i for i, f in enumerate(frames)]
        self.sums = [(0x9E3779B1 * (i + 1)) & 0xFFFFFFFF for i in range(len(frames))] if cks else None
        self.recs = sk.records([len(f) for f in frames], self.sizes, self.sums) if recs is None else recs
        if spoil:
            spoil(self.recs)
        self.cap = model.bound(sum(map(len, frames)), len(frames), cks) if cap is None else cap

    @property
    def blob(self):
        return sk.pack_case(self.frames, self.recs, flags=self.flags, cap=self.cap, residue=self.residue)


def pack_cases():
    """name -> PackCase"""
    c = {}
    # lengths 1..40, each at all 16 source residues (frame i sits i % 16 bytes into its block), the stream at all 16 residues
    cyc = blobs([1 + (i // 16) % 40 for i in range(640)], 1)
    for r in range(16):
        c[f"cyclic_{r}"] = PackCase(cyc, cks=bool(r & 1), residue=r)
    for n in COUNTS:
        c[f"count_{n}"] = PackCase(blobs([(7 * i) % 41 for i in range(n)], n), cks=bool(n & 1), residue=n % 16)
    c["three_tiles_and_a_byte"] = PackCase(blobs([3, 9, 3 * TILE + 1, 1, 2, 40, 17], 3), cks=True, residue=5)
    for r in (0, 7):                                                    # the second frame ends exactly where the first tile ends
        c[f"ends_on_a_tile_{r}"] = PackCase(blobs([5, TILE - 5 - r, 33, 2 * TILE - 33, 6], 4), residue=r)
    c["past_65535"] = PackCase(blobs([1 + i % 3 for i in range(70000)], 5), residue=3)
    few = blobs([30, 0, 17, 200, 1], 6)
    need = model.bound(sum(map(len, few)), 5, True)
    c["cap_exact_plus"] = PackCase(few, cks=True, residue=2, cap=need + 5)
    c["cap_exact"] = PackCase(few, cks=True, residue=2, cap=need)
    c["cap_short"] = PackCase(few, cks=True, residue=2, cap=need - 1, expect=(model.TOO_SMALL, 0, need))
    for name, i in (("first", 0), ("middle", 2), ("last", 4)):
        def fail(recs, i=i):
            recs["status"][i] = 900
        c[f"failed_{name}"] = PackCase(few, residue=1, spoil=fail, expect=(model.INVALID_ARG, i, 0))

    def two_bad(recs):
        recs["bytes_read"][3] = 1 << 32
        recs["bytes_written"][1] = 1 << 32
    c["two_sizes_too_large"] = PackCase(few, residue=1, spoil=two_bad, expect=(model.INVALID_ARG, 1, 0))

    def no_sum(recs):
        recs["flags"][3] = 64
    c["one_without_checksum"] = PackCase(few, cks=True, spoil=no_sum, expect=(model.INVALID_ARG, 3, 0))
    # three records of 0xFFE00000 bytes over empty slots and no room at all: the need in 64 bits, nothing read, nothing touched
    c["huge"] = PackCase([b""] * 3, cap=0, residue=9, recs=sk.records([HUGE] * 3, [HUGE] * 3), expect=(model.TOO_SMALL, 0, 3 * HUGE + 8 + 24 + 9))
    return c


REFUSED = ("cap_short", "failed_first", "failed_middle", "failed_last", "two_sizes_too_large", "one_without_checksum", "huge")


class OpenCase:
    """A stream, a range, and what an open must give: `want` is (status, the five arrays, the bytes the range needs) or the reason of
    the table's defect; `inf` the model's cz_seekable_info."""

    def __init__(self, stream, first, count, align, k, want, arrays=True, residue=1):
        self.stream, self.first, self.count, self.align, self.k, self.want, self.arrays, self.residue = stream, first, count, align, k, want, arrays, residue
        self.inf = model.info_of(stream)

    @property
    def blob(self):
        return sk.open_case(self.stream, self.first, self.count, self.align, k=self.k, arrays=self.arrays, residue=self.residue)


def open_cases():
    out = []
    for n, cks in ((0, False), (1, True), (2, False), (300, True), (300, False), (257, True), (4097, True)):
        frames = blobs([(11 * i) % 41 for i in range(n)], 20 + n)
        stream = model.build(frames, [5 * len(f) + 1 for f in frames], [i * 0x01000193 & 0xFFFFFFFF for i in range(n)] if cks else None)
        ranges = [(0, n), (n, 0), (3, 5), (0, sk.ALL), (n + 1, 0), (n + 1, sk.ALL), (0, n + 1)] + ([(n - 1, 1)] if n else [])
        for j, (first, count) in enumerate(ranges):
            align = (1, 16, 256)[j % 3]
            st, *arrays, need = model.open_range(stream, first, None if count == sk.ALL else count, align)
            out.append(OpenCase(stream, first, count, align, len(arrays[0]), (st, arrays, need), residue=1 + j))
        out.append(OpenCase(stream, 0, sk.ALL, 1, 0, (0, [[]] * 5, model.open_range(stream)[-1]), arrays=False))
        if n == 300:
            for reason, s in list(model.damaged(stream).items()) + model.damaged_more(stream):
                out.append(OpenCase(s, 0, sk.ALL, 1, 300 if reason != 1 else 0, reason))
    return out


def check_open(i, c, info, arrays):
    """One open's info record and arrays (k entries each, 0xA5 where nothing was written) against the case."""
    if isinstance(c.want, int):
        assert (int(info["status"]), int(info["reason"])) == (model.SEEK_TABLE, c.want), i
        assert all(int(info[k]) == v for k, v in c.inf.items()), i
        assert all(set(a.tobytes()) <= {0xA5} for a in arrays), f"case {i}: an array was written on a table error"
        return
    st, want, need = c.want
    assert int(info["status"]) == st, i
    for k, v in c.inf.items():
        if k != "status":
            assert int(info[k]) == v, (i, k)
    if st == 0:
        assert [a.tolist() for a in arrays] == [list(a) for a in want] and int(info["detail"]) == need, i
    else:
        assert int(info["detail"]) == 0 and all(a.size == 0 for a in arrays), i


def check_good(name, c, info, block):
    """A pack that must go well: the block is poison up to the stream, the model's stream, poison behind it.  Returns the stream."""
    want = model.build(c.frames, c.sizes, c.sums)
    assert int(info["status"]) == 0, (name, int(info["status"]))
    assert block[:c.residue] == b"\xEE" * c.residue, f"{name}: bytes in front of the stream were touched"
    assert block[c.residue:c.residue + len(want)] == want, f"{name}: the stream differs from the model's"
    assert set(block[c.residue + len(want):]) <= {0xEE}, f"{name}: bytes past stream_bytes were touched"
    got = {k: int(info[k]) for k in ("reason", "frames", "frames_bytes", "content_bytes", "stream_bytes", "detail", "has_checksums", "reserved")}
    assert got == dict(reason=0, frames=len(c.frames), frames_bytes=sum(map(len, c.frames)), content_bytes=sum(c.sizes), stream_bytes=len(want),
                       detail=0, has_checksums=c.flags, reserved=0), name
    return want


def check_refused(name, c, info, block):
    status, detail, need = c.expect
    assert int(info["status"]) == status, (name, int(info["status"]))
    assert int(info["detail"]) == detail and int(info["stream_bytes"]) == need and int(info["reason"]) == 0, name
    assert set(block) <= {0xEE}, f"{name}: the stream was touched"
    if name == "huge":
        assert int(info["frames_bytes"]) == int(info["content_bytes"]) == 3 * HUGE > 1 << 33


@pytest.fixture(scope="module")
def packed():
    """name -> (the case, the emulator's result, the host function's result)"""
    cases = pack_cases()
    blob = [c.blob for c in cases.values()]
    emu = sk.run(sk.EMU, blob)
    assert emu[0] == TILE
    host = sk.run(sk.HOST, blob)
    return {name: (c, e, h) for (name, c), e, h in zip(cases.items(), emu[1:], host)}


def good(packed, name):
    c, (_, info, block), (ret, hinfo, hblock) = packed[name]
    assert ret == 0 and info.tobytes() == hinfo.tobytes(), name
    assert block == hblock, f"{name}: the kernels' stream differs from cz_seekable_pack_host's"
    return check_good(name, c, info, block)


@pytest.mark.parametrize("r", range(16))
def test_every_length_at_every_source_and_destination_residue(packed, r):
    good(packed, f"cyclic_{r}")


@pytest.mark.parametrize("n", COUNTS)
def test_frame_counts_around_the_wave_and_the_workgroup(packed, n):
    want = good(packed, f"count_{n}")
    assert n or len(want) == 17


def test_large_frames_across_tiles(packed):
    good(packed, "three_tiles_and_a_byte")
    good(packed, "ends_on_a_tile_0")
    good(packed, "ends_on_a_tile_7")


def test_indices_past_65535(packed):
    want = good(packed, "past_65535")
    reason, ents = model.parse(want)
    assert reason == 0 and len(ents) == 70000 and ents[65536][0] == 1 + 65536 % 3


def test_stream_cap_at_the_need(packed):
    good(packed, "cap_exact")
    good(packed, "cap_exact_plus")


@pytest.mark.parametrize("name", REFUSED)
def test_refusals_touch_nothing(packed, name):
    c, (_, info, block), (ret, hinfo, hblock) = packed[name]
    assert ret == c.expect[0] and info.tobytes() == hinfo.tobytes() and block == hblock, name
    check_refused(name, c, info, block)
    assert name != "huge" or len(block) == 9


def test_open_on_the_models_streams():
    cases = open_cases()
    blob = [c.blob for c in cases]
    emu, host = sk.run(sk.EMU, blob)[1:], sk.run(sk.HOST, blob)
    for i, (c, e, h) in enumerate(zip(cases, emu, host)):
        assert e[1].tobytes() == h[1].tobytes() and int(e[1]["status"]) == h[0], i
        assert all(a.tobytes() == b.tobytes() for a, b in zip(e[2:], h[2:])), i
        check_open(i, c, e[1], e[2:])


def test_open_a_range_past_index_65535(packed):
    stream = good(packed, "past_65535")
    st, *arrays, need = model.open_range(stream, 65500, 300, 16)
    (emu,) = sk.run(sk.EMU, [sk.open_case(stream, 65500, 300, 16, k=300, residue=3)])[1:]
    assert int(emu[1]["status"]) == 0 and [a.tolist() for a in emu[2:]] == arrays and int(emu[1]["detail"]) == need
    assert int(emu[1]["frames"]) == 70000
