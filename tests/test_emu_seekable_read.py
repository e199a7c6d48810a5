"""The seekable-read kernels (cz_seekable_index_kernel, cz_seekable_locate_kernel, cz_seekable_select_kernel,
cz_seekable_ranges_kernel; the unmodified czstd_seekable_read.hip) on the CPU SIMT emulator under ASan + UBSan
(tests/emu/emu_seekable_read.cpp).  The index's arrays and scratch, every array of a locate, the decoded buffer and the destination
sit in exact-size heap blocks; arrays start as 0xA5, the destination as 0xEE, and the decoded buffer is the contents laid at out_off
with 0xEE in the alignment gaps, so no decoder is needed.  What comes out is compared with the model (seekable_read_model.py) and,
byte for byte and field for field, with cz_seekable_locate_host / cz_seekable_gather_host run on the same case file
(tests/emu/seekable_read_host_main.cpp).  The emulator runs workgroups one after another, so this checks formats and bookkeeping
(selection, spans, bounds, a clean scratch), not concurrency between the workgroups of the range kernel or the gather.  No GPU
needed.  Every test here fails without the feature: the kernels and the driver do not exist."""
import numpy as np
import pytest

import seekable_model as fmt
import seekable_read_model as model
import seekable_read_runner as sr

pytestmark = pytest.mark.xdist_group(name="emu_seekable_read")
TILE = 8192                                                              # the gather's tile (checked against what the binary reports)
N_COUNTS = (0, 1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097)        # frames: around a thread's share, a wave, a workgroup, a scan tile
M_COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 4097)                    # ranges: around a wave, a workgroup of the range kernel, a scan tile
HUGE = 0xFFE00000
U64 = (1 << 64) - 1


def table(sizes, cks=False):
    """A stream whose table lists frames of these decompressed sizes (the frames themselves are one to three bytes of anything)."""
    frames = [bytes([i & 255]) * (1 + i % 3) for i in range(len(sizes))]
    return fmt.build(frames, sizes, [i * 0x01000193 & 0xFFFFFFFF for i in range(len(sizes))] if cks else None)


def cycling(n):
    return [(7 * i) % 41 for i in range(n)]                             # 0..40, zeros included


def some_ranges(sizes, m, seed):
    """m ranges inside the content: short ones, some empty, a few long, offsets anywhere (the content's end included)."""
    content, rng = sum(sizes), np.random.default_rng(seed)
    out = []
    for j in range(m):
        o = int(rng.integers(0, content + 1))
        ln = 0 if j % 7 == 3 else int(rng.integers(1, 500)) if j % 31 == 5 else int(rng.integers(1, 60))
        out.append((o, min(ln, content - o)))
    return out


class Call:
    """One locate: frames_cap None: what the model selects; the blocks of the per-frame arrays hold min(selected, frames_cap) entries."""

    def __init__(self, ranges, align=1, frames_cap=None, arrays=True):
        self.ranges, self.align, self.frames_cap, self.arrays = list(ranges), align, frames_cap, arrays

    def resolve(self, stream):
        self.want = model.locate(stream, self.ranges, self.align, self.frames_cap, per_frame=self.arrays)
        k = self.want[0]["selected"]
        self.cap = k if self.frames_cap is None else self.frames_cap
        self.k = min(k, self.cap) if self.arrays else 0
        return sr.call(self.ranges, self.align, self.cap, self.k, self.arrays)


class LocateCase:
    def __init__(self, stream, calls=()):
        self.stream, self.calls = stream, list(calls)
        self.inf = fmt.info_of(stream)

    @property
    def blob(self):
        return sr.locate_case(self.stream, [c.resolve(self.stream) for c in self.calls])


def edge_sizes():
    #        0  1  2   3  4  5  6  7  8   9  10 11 12      content: 3 [0,10) 4 [10,15) 6 [15,22) 9 [22,42) 10 [42,58)
    return [0, 0, 0, 10, 5, 0, 7, 0, 0, 20, 16, 0, 0]


EDGE_RANGES = {
    "whole": (0, 58), "empty_at_0": (0, 0), "empty_at_the_end": (58, 0), "empty_between_frames": (10, 0),
    "first_byte_of_a_frame": (10, 1), "last_byte_of_a_frame": (14, 1), "ends_on_a_boundary": (3, 7), "starts_on_a_boundary": (15, 3),
    "two_frames_around_an_empty_one": (12, 5), "three_frames_and_empty_ones": (12, 12), "behind_empty_frames_at_the_start": (0, 1),
    "in_front_of_empty_frames_at_the_end": (57, 1), "behind_a_run_of_empty_frames": (22, 1),
}
EDGE_SELECTS = {
    "whole": [3, 4, 6, 9, 10], "empty_at_0": [], "empty_at_the_end": [], "empty_between_frames": [], "first_byte_of_a_frame": [4],
    "last_byte_of_a_frame": [4], "ends_on_a_boundary": [3], "starts_on_a_boundary": [6], "two_frames_around_an_empty_one": [4, 6],
    "three_frames_and_empty_ones": [4, 6, 9], "behind_empty_frames_at_the_start": [3], "in_front_of_empty_frames_at_the_end": [10],
    "behind_a_run_of_empty_frames": [9],
}


def locate_cases():
    """name -> LocateCase"""
    c = {}
    for q, n in enumerate(N_COUNTS):
        sizes = cycling(n)
        content = sum(sizes)
        m = M_COUNTS[(q + 3) % len(M_COUNTS)] if content else 3
        ranges = some_ranges(sizes, m, 100 + n)
        c[f"frames_{n}"] = LocateCase(table(sizes, cks=bool(n & 1)), [
            Call(ranges, align=(1, 16, 256)[q % 3], arrays=False), Call(ranges, align=(1, 16, 256)[q % 3]),
            Call([(0, content)], align=16), Call([])])
    sizes = cycling(300)
    for q, m in enumerate(M_COUNTS):
        c[f"ranges_{m}"] = LocateCase(table(sizes, cks=bool(q & 1)), [Call(some_ranges(sizes, m, 200 + m), align=(256, 1, 16)[q % 3])])
    edges = list(EDGE_RANGES.values())
    c["edges"] = LocateCase(table(edge_sizes(), cks=True), [Call([r], align=16) for r in edges]
                            + [Call(edges), Call(edges[::-1], align=256), Call(edges + edges + [(5, 30), (20, 30), (0, 58)])])
    many = cycling(4300)
    c["one_range_over_4300_frames"] = LocateCase(table(many), [Call([(5, sum(many) - 45)], align=16)])
    # the first locate covers everything, the second one byte: it must select one frame, whatever the first left behind
    c["two_locates"] = LocateCase(table(many, cks=True), [Call([(0, sum(many))]), Call([(sum(many[:2000]) + 1, 1)]), Call([(0, sum(many))], arrays=False),
                                                          Call([(3, 1)])])
    content = sum(sizes)
    good = some_ranges(sizes, 9, 7)
    long = (content - 3, 4)                                             # one byte too long
    k = model.locate(table(sizes), good)[0]["selected"]
    c["refusals"] = LocateCase(table(sizes), [
        Call([long] + good), Call(good), Call(good[:4] + [long] + good[4:]), Call(good, align=16), Call(good + [long]), Call(good),
        Call(good[:2] + [long] + good[2:5] + [(content + 1, 0)] + good[5:]), Call(good), Call([(U64, 2)] + good), Call(good),
        Call(good + [(3, U64)]), Call(good), Call(good, frames_cap=k - 1), Call(good, frames_cap=k), Call(good, frames_cap=0, arrays=False),
        Call(good, frames_cap=k - 1, align=256), Call(good)])
    huge = table([HUGE] * 3, cks=True)
    c["above_4_gib"] = LocateCase(huge, [
        Call([(HUGE + 5, 10), (2 * HUGE - 3, 6), (3 * HUGE, 0), ((1 << 32) + 1, 1), (5, 1)], align=4096), Call([(0, 3 * HUGE)], align=4096),
        Call([(2 * HUGE + 7, HUGE - 7)]), Call([(3 * HUGE, 1)]), Call([(2 * HUGE, 1)])])
    return c


def damaged_cases():
    stream = table(cycling(300), cks=True)
    return [(reason, LocateCase(s)) for reason, s in list(fmt.damaged(stream).items()) + fmt.damaged_more(stream)]


def check_call(name, q, call, ret, info, clean, arrays, spans):
    """One locate's return value, info record, arrays and spans (0xA5 where nothing was written) against the model."""
    winfo, warrays, wspans = call.want
    at = f"{name}[{q}]"
    assert ret == winfo["status"] == int(info["status"]), (at, ret, winfo["status"])
    assert {k: int(info[k]) for k in winfo} == winfo, at
    assert clean == 1, f"{at}: the scratch was not clean after the call"
    if winfo["status"] == 0 and call.arrays:
        assert [a.tolist() for a in arrays] == [warrays[k] for k in model.ARRAYS], at
        assert [tuple(int(x) for x in sp) for sp in spans] == wspans, at
    else:
        assert all(set(a.tobytes()) <= {0xA5} for a in arrays) and set(spans.tobytes()) <= {0xA5}, f"{at}: an array was written"


@pytest.fixture(scope="module")
def located():
    """name -> (the case, the emulator's result, the host program's result)"""
    cases = locate_cases()
    blob = [c.blob for c in cases.values()]
    emu = sr.run(sr.EMU, blob)
    assert emu[0] == TILE
    host = sr.run(sr.HOST, blob)
    return {name: (c, e, h) for (name, c), e, h in zip(cases.items(), emu[1:], host)}


def check_located(located, name):
    c, (ret, tab, calls), (hret, htab, hcalls) = located[name]
    assert ret == hret == 0 and tab.tobytes() == htab.tobytes(), name
    assert all(int(tab[k]) == v for k, v in c.inf.items()) and int(tab["detail"]) == 0, name
    assert len(calls) == len(hcalls) == len(c.calls)
    for q, (call, e, h) in enumerate(zip(c.calls, calls, hcalls)):
        check_call(name, q, call, *e)
        assert e[0] == h[0] and e[1].tobytes() == h[1].tobytes(), f"{name}[{q}]: the kernels' info differs from cz_seekable_locate_host's"
        assert all(a.tobytes() == b.tobytes() for a, b in zip(e[3], h[3])) and e[4].tobytes() == h[4].tobytes(), f"{name}[{q}]: arrays differ from the host's"
    return c, calls


@pytest.mark.parametrize("n", N_COUNTS)
def test_frame_counts_around_the_wave_the_workgroup_and_the_scan_tile(located, n):
    c, calls = check_located(located, f"frames_{n}")
    assert int(calls[0][1]["selected"]) == int(calls[1][1]["selected"]) and int(calls[3][1]["selected"]) == 0
    assert int(calls[2][1]["selected"]) == sum(1 for s in cycling(n) if s)   # the whole content: every frame that is not empty


@pytest.mark.parametrize("m", M_COUNTS)
def test_range_counts_around_the_wave_and_the_workgroup(located, m):
    check_located(located, f"ranges_{m}")


def test_ranges_at_the_edges_of_frames(located):
    c, calls = check_located(located, "edges")
    for (name, want), got in zip(EDGE_SELECTS.items(), calls):
        assert got[3][0].tolist() == want, name
    assert calls[-1][3][0].tolist() == [3, 4, 6, 9, 10]                  # duplicates and overlaps: each frame once


def test_one_range_over_more_frames_than_a_scan_tile(located):
    c, calls = check_located(located, "one_range_over_4300_frames")
    sizes = cycling(4300)
    assert int(calls[0][1]["selected"]) == sum(1 for s in sizes if s) - 1 > 4097   # (the last frame holds none of its bytes)


def test_two_locates_on_one_index_do_not_see_each_other(located):
    c, calls = check_located(located, "two_locates")
    assert int(calls[1][1]["selected"]) == 1 and calls[1][3][0].tolist() == [2000]
    assert int(calls[3][1]["selected"]) == 1


def test_refusals_write_nothing_and_leave_the_index_clean(located):
    c, calls = check_located(located, "refusals")
    got = [(r, int(i["detail"])) for r, i, *_ in calls]
    assert got[0] == (model.INVALID_ARG, 0) and got[2] == (model.INVALID_ARG, 4) and got[4] == (model.INVALID_ARG, 9)
    assert got[6] == (model.INVALID_ARG, 2) and got[8] == (model.INVALID_ARG, 0) and got[10] == (model.INVALID_ARG, 9)
    assert got[12][0] == model.TOO_SMALL and got[13][0] == 0 and got[14][0] == 0 and got[15][0] == model.TOO_SMALL
    assert all(got[q][0] == 0 for q in (1, 3, 5, 7, 9, 11, 16))         # a clean locate directly after each refusal
    assert int(calls[12][1]["selected"]) == int(calls[13][1]["selected"]) == c.calls[13].k


def test_offsets_above_4_gib(located):
    c, calls = check_located(located, "above_4_gib")
    assert calls[0][3][0].tolist() == [0, 1, 2] and int(calls[0][1]["content_bytes"]) == 3 * HUGE > 1 << 33
    assert calls[0][3][3].tolist() == [0, HUGE, 2 * HUGE]              # out_off at out_align 4096
    assert calls[2][3][0].tolist() == [2] and calls[3][0] == model.INVALID_ARG and calls[4][3][0].tolist() == [2]


def test_index_refuses_a_damaged_table_with_each_reason():
    cases = damaged_cases()
    blob = [c.blob for _, c in cases]
    emu, host = sr.run(sr.EMU, blob)[1:], sr.run(sr.HOST, blob)
    assert sorted({r for r, _ in cases}) == list(fmt.REASONS)
    for (reason, c), (ret, tab, calls), (hret, htab, _) in zip(cases, emu, host):
        assert ret == hret == model.SEEK_TABLE and int(tab["reason"]) == reason and tab.tobytes() == htab.tobytes(), reason
        assert all(int(tab[k]) == v for k, v in c.inf.items()) and calls == [], reason


# ---- gather -------------------------------------------------------------------------------------------------------------------

def blobs(lengths, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lengths]


class GatherCase:
    """Contents, ranges and a destination residue: the arrays and spans come from the model, the decoded buffer is the contents at
    out_off with 0xEE in the gaps; `want` is the slices of the content back to back."""

    def __init__(self, contents, ranges, residue=0, align=1):
        self.contents, self.ranges, self.residue, self.align = contents, list(ranges), residue, align
        info, self.arrays, spans = model.locate_entries([(1, len(b), None) for b in contents], self.ranges, align)
        assert info["status"] == 0
        self.info, self.spans = info, sr.spans_array(spans)
        self.decoded = model.decoded(contents, self.arrays, info["out_bytes"])
        self.want = model.gathered(contents, self.ranges)
        assert len(self.want) == info["dst_bytes"]

    @property
    def blob(self):
        return sr.gather_case(self.arrays["out_off"], self.arrays["content_off"], self.decoded, self.ranges, self.spans, len(self.want), self.residue)


def gather_cases():
    """name -> GatherCase"""
    c = {}
    # ranges of 1..40 bytes whose offsets walk through all 16 source residues, the destination at all 16 residues; the frames are
    # shorter than many of the ranges, and some are empty
    frames = blobs([(11 * i) % 37 for i in range(700)], 31)
    content = sum(map(len, frames))
    for r in range(16):
        c[f"cyclic_{r}"] = GatherCase(frames, [((j * 17 + r) % (content - 40), 1 + (j // 16) % 40) for j in range(640)], residue=r, align=(1, 16)[r & 1])
    big = blobs([3, 40000, 0, 9, 25, 30000], 32)
    c["three_tiles_and_a_byte"] = GatherCase(big, [(0, 3), (1, 9), (7, 3 * TILE + 1), (40010, 1), (5, 2), (40020, 40), (3, 17)], residue=5)
    for r in (0, 7):                                                    # the second range ends exactly where the first tile ends
        c[f"ends_on_a_tile_{r}"] = GatherCase(big, [(1, 5), (20, TILE - 5 - r), (100, 33), (40050, 2 * TILE - 33), (2, 6)], residue=r)
    few = blobs([30, 0, 17, 200, 1], 33)
    c["empty_ranges"] = GatherCase(few, [(0, 0), (5, 0), (3, 40), (47, 0), (248, 0), (46, 3), (10, 0), (0, 248), (248, 0), (7, 0)], residue=3)
    c["only_empty_ranges"] = GatherCase(few, [(0, 0), (248, 0)], residue=1)
    c["no_ranges"] = GatherCase(few, [], residue=2)
    tiny = blobs([1 + i % 5 for i in range(400)], 34)
    total = sum(map(len, tiny))
    c["past_65535"] = GatherCase(tiny, [((j * 7) % (total - 3), 1 + j % 3) for j in range(70000)], residue=3)
    gaps = blobs([100, 300, 0, 7, 260, 0, 0, 50], 35)                   # out_align 256: gaps in the source between the frames
    c["across_frames_with_gaps"] = GatherCase(gaps, [(90, 20), (95, 310), (399, 8), (400, 270), (0, 717), (660, 57), (100, 1), (99, 2)], residue=9, align=256)
    return c


def check_gathered(name, c, block):
    assert block[:c.residue] == b"\xEE" * c.residue, f"{name}: bytes in front of the destination were touched"
    assert block[c.residue:c.residue + len(c.want)] == c.want, f"{name}: the gathered bytes differ from the slices of the content"
    assert set(block[c.residue + len(c.want):]) <= {0xEE}, f"{name}: bytes past dst_bytes were touched"


@pytest.fixture(scope="module")
def gathered():
    cases = gather_cases()
    blob = [c.blob for c in cases.values()]
    emu, host = sr.run(sr.EMU, blob)[1:], sr.run(sr.HOST, blob)
    return {name: (c, e, h) for (name, c), e, h in zip(cases.items(), emu, host)}


def good(gathered, name):
    c, (_, block), (hret, hblock) = gathered[name]
    assert hret == 0 and len(block) == c.residue + len(c.want), name
    assert block == hblock, f"{name}: the kernel's bytes differ from cz_seekable_gather_host's"
    check_gathered(name, c, block)
    return c


@pytest.mark.parametrize("r", range(16))
def test_every_length_at_every_source_and_destination_residue(gathered, r):
    good(gathered, f"cyclic_{r}")


def test_large_ranges_across_tiles(gathered):
    good(gathered, "three_tiles_and_a_byte")
    good(gathered, "ends_on_a_tile_0")
    good(gathered, "ends_on_a_tile_7")


def test_empty_ranges_first_last_and_between(gathered):
    good(gathered, "empty_ranges")
    good(gathered, "only_empty_ranges")
    good(gathered, "no_ranges")


def test_range_indices_past_65535(gathered):
    c = good(gathered, "past_65535")
    assert len(c.ranges) == 70000


def test_ranges_across_two_and_three_frames_with_gaps_in_the_source(gathered):
    c = good(gathered, "across_frames_with_gaps")
    assert c.arrays["out_off"] == [0, 256, 768, 1024, 1536] and [int(x) for x in c.spans["sel_count"][:5]] == [2, 3, 2, 3, 5]
