"""CZ_COMPRESS_HIGH_SPLIT (cz_compress_plan_kernel and cz_compress_segments_high_kernel; the kernel sources unmodified) on the CPU SIMT
emulator under ASan + UBSan (tests/emu/emu_encode_high_split.cpp), built with one-block segments (S = 128 KiB) and an 8 KiB overlap.
The emulator runs workgroups one after another, so this checks the frame format and the chain bookkeeping, not concurrency
(tests/test_compress_high_split_gpu.py does that).  Every frame must decode to its input under the oracle (status 0, every byte
consumed, content size) and under libzstd where the host has it, stay within cz_compress_bound, leave 0xEE past bytes_written, carry
Last_Block once and result flags 512 | checksum.  The model of the offset history and the reach check of tests/compress_high_split.py
run on every frame of more than one segment.  No GPU needed."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import compress_edges as ce
import compress_frames as cf
import compress_high_split as hs
import emu_encode_high_split_runner as emu
import oracle
from compress_split import blocks_of, text

pytestmark = pytest.mark.xdist_group(name="emu_encode_high_split")
S, W, BLOCK = emu.S, emu.W, 128 << 10
TOO_SMALL = 900
HS, H, SF, CK = emu.HIGH_SPLIT, emu.HIGH, emu.SPLIT | emu.FSE_TABLES, emu.CHECKSUM
TYPES = {0: "raw", 1: "rle", 2: "compressed"}


def check(name, b, r, region, flags):
    assert int(r["status"]) == 0, name
    n = int(r["bytes_written"])
    frame = region[:n]
    assert n <= emu.compress_bound(len(b)) == len(region), (name, n)
    assert set(region[n:]) <= {0xEE}, f"{name}: bytes past bytes_written were touched"
    assert int(r["bytes_read"]) == len(b) and int(r["blocks"]) == max(1, -(-len(b) // BLOCK)), name
    assert int(r["flags"]) == flags, (name, int(r["flags"]))
    st, out, info = oracle.decode_frame(frame, cap=len(b) + 64)
    assert st == 0 and out == b and info["consumed"] == n, (name, st)
    assert info["content_size"] == len(b)
    if flags & CK:
        assert info["has_checksum"] and info["checksum"] == oracle.xxh64(b) & 0xFFFFFFFF == int(r["checksum"]), name
    if cf.libzstd():
        assert cf.libzstd_decompress(frame, len(b)) == b, f"{name}: libzstd"
    hl, blocks = blocks_of(frame)
    assert [last for _, last, _, _, _ in blocks] == [0] * (len(blocks) - 1) + [1], name
    assert len(blocks) == int(r["blocks"])
    if flags & HS and len(b) > S:                                       # more than one segment
        an = ce.analyse(frame, b)
        hs.check_history(an, S)
        hs.check_reach(an, S, W)
    return frame


@pytest.fixture(scope="module")
def built():
    return {"two_offsets_across_cuts": hs.two_offsets_across_cuts(S), "long_match_in_overlap": hs.long_match_in_overlap(S, W)}


@pytest.fixture(scope="module")
def runs(built):
    """Every emulator run of this file, four at a time (each is one mostly serial program): name -> (inputs, flags, results)."""
    rng = np.random.default_rng(99)
    T = text(2 * S + 70001)
    two, far = built["two_offsets_across_cuts"].data, built["long_match_in_overlap"].data
    capin = b"\0" * S + text(S, skip=777) + text(5000, skip=31)         # 3 segments: an RLE block, a Compressed one, a short tail
    small = text(3000, skip=5)
    short = [b"", b"\x41", T[:15], T[:16], T[:S - 1], T[:S]]
    around = [T[:S + 1], T[:S + 5], T[:S + 8], T[:S + 16], T[:2 * S], T]
    mix = [small, far, b"", T[:S + 16], T[:20000]]                      # one-unit and many-unit frames
    jobs = {
        "short": (short, HS), "short_high": (short, H),
        "around": (around, HS), "around_high": (around, H),
        "pieces_high": ([T[S:S + 1], T[S:S + 5], T[S:S + 8], T[S:S + 16], T[S:2 * S], T[2 * S:]], H),
        "special": ([b"\0" * (3 * S), rng.bytes(2 * S), rng.bytes(S) + text(40000, skip=123)], HS),
        "constructed": ([two, far], HS), "two_high": ([two], H), "far_split_fse": ([far], SF),
        "checksum": ([T[:S + 1], capin, b"", small], HS | CK),
        "cap_full": ([capin, small], HS),
        "mix": (mix, HS), "mix_reversed": (mix[::-1], HS),
    }
    emu.build()
    with ThreadPoolExecutor(4) as ex:
        fut = {k: ex.submit(emu.run, bufs, flags=flags) for k, (bufs, flags) in jobs.items()}
        got = {k: (jobs[k][0], jobs[k][1], f.result()) for k, f in fut.items()}
    # the out_cap runs need the full frame's layout first
    full = got["cap_full"][2][0]
    need = int(full[0]["bytes_written"])
    hl, blocks = blocks_of(full[1][:need])
    caps = {"hdr-1": (hl - 1, HS), "hdr": (hl, HS), "full": (need, HS), "full_ck-1": (need + 3, HS | CK), "full_ck": (need + 4, HS | CK)}
    for j, (at, _, _, _, size) in enumerate(blocks):
        caps[f"end{j}-1"] = (at + size - 1, HS)
        if j + 1 < len(blocks):
            caps[f"end{j}"] = (at + size, HS)
    with ThreadPoolExecutor(4) as ex:
        fut = {k: ex.submit(emu.run, [capin, small], caps=[c, emu.compress_bound(len(small))], flags=flags) for k, (c, flags) in caps.items()}
        for k, f in fut.items():
            got[("cap", k)] = ([capin, small], caps[k], f.result())
    return got


def frames(runs, key):
    bufs, flags, res = runs[key]
    return [check(f"{key}[{i}]", b, r, region, flags) for i, (b, (r, region)) in enumerate(zip(bufs, res))]


def test_up_to_one_segment_is_the_high_frame(runs):
    """Lengths 0, 1, 15, 16, S - 1 and S: byte for byte the frames of cz_compress_frames_high_kernel; flags 512."""
    assert frames(runs, "short") == frames(runs, "short_high")


def test_lengths_around_a_cut(runs):
    """S + 1, S + 5 (a Raw tail below 16 bytes), S + 8, S + 16, 2 S and 2 S + 70 001 bytes of corpus text: one block per 128 KiB,
    the types of the short tails, header and segment 0 byte for byte the CZ_COMPRESS_HIGH frame's, and the frame no larger than the
    CZ_COMPRESS_HIGH frames of its segments compressed alone."""
    split, high, pieces = frames(runs, "around"), frames(runs, "around_high"), frames(runs, "pieces_high")
    whole = frames(runs, "short_high")[5]                               # T[:S]
    tails = {S + 1: ("rle",), S + 5: ("raw",), S + 8: ("raw",), S + 16: ("raw", "compressed"), 2 * S: ("compressed",), 2 * S + 70001: ("compressed",)}
    for i, (b, fs, fh) in enumerate(zip(runs["around"][0], split, high)):
        hl, blocks = blocks_of(fs)
        types = [TYPES[bt] for _, _, bt, _, _ in blocks]
        print(f"{len(b)} bytes: {types}, {len(fs)} bytes against {len(fh)} unsplit")
        assert len(blocks) == -(-len(b) // BLOCK) and types[0] == "compressed" and types[-1] in tails[len(b)], (len(b), types)
        if len(b) > 2 * S:
            assert types[1] == "compressed"
        seg0 = blocks[0][0] + blocks[0][4]                              # header and the one block of segment 0
        assert hl == blocks_of(fh)[0] and fs[:seg0] == fh[:seg0]
        alone = [whole, pieces[min(i, 4)]] + ([pieces[5]] if len(b) > 2 * S else [])
        assert len(fs) <= sum(map(len, alone)), (len(b), len(fs), [len(p) for p in alone])


def test_rle_raw_and_history_behind_raw(runs):
    zeros, rnd, rnd_text = frames(runs, "special")
    assert [t for t, _ in cf.walk(zeros)] == ["rle"] * 3
    assert [t for t, _ in cf.walk(rnd)] == ["raw"] * 2
    # a Raw segment 0, then text: the later segment starts from a history of its own (check() ran the model on it)
    assert [t for t, _ in cf.walk(rnd_text)] == ["raw", "compressed"]


def test_two_offsets_across_cuts(runs, built):
    """Every later segment starts explicit and then writes Offset_Values 2 or 3; the unsplit frame has a repeat code behind each cut."""
    b = built["two_offsets_across_cuts"]
    fs = frames(runs, "constructed")[0]
    hs.expect_two_offsets_across_cuts(ce.analyse(fs, b.data), b, S)
    (fh,) = frames(runs, "two_high")
    hs.expect_two_offsets_across_cuts(ce.analyse(fh, b.data), b, S, split=False)
    assert fs[:blocks_of(fs)[1][1][0]] == fh[:blocks_of(fh)[1][1][0]]   # segment 0


def test_long_match_in_overlap(runs, built):
    """The second table is warmed from the overlap: the long match behind the cut is found with its far offset; the frame of
    CZ_COMPRESS_SPLIT | CZ_COMPRESS_FSE_TABLES, with its one table, has the short one."""
    b = built["long_match_in_overlap"]
    hs.expect_long_match_in_overlap(ce.analyse(frames(runs, "constructed")[1], b.data), b)
    hs.expect_long_match_in_overlap(ce.analyse(frames(runs, "far_split_fse")[0], b.data), b, found=False)


def test_checksum(runs):
    """The checksum of a frame of several segments comes from its checksum unit, that of a short one from its own workgroup (check
    compares both with the oracle's); the result flags are 513 for all."""
    frames(runs, "checksum")
    assert [int(r["flags"]) for r, _ in runs["checksum"][2]] == [HS | CK] * 4


def test_output_too_small_is_a_block_aligned_prefix(runs):
    """out_cap of header - 1, header, each block's end - 1 and exact, full - 1 with the checksum, and full: the frame is the whole
    blocks that fit, the fields cover them, nothing past bytes_written is touched and the neighbour frame is intact."""
    full, neighbour = frames(runs, "cap_full")
    hl, blocks = blocks_of(full)
    assert [TYPES[bt] for _, _, bt, _, _ in blocks] == ["rle", "compressed", "compressed"]
    ends = [at + size for at, _, _, _, size in blocks]
    placed = {"hdr-1": 0, "hdr": 0, "end0-1": 0, "end0": 1, "end1-1": 1, "end1": 2, "end2-1": 2}
    seen = 0
    for key, run in runs.items():
        if not isinstance(key, tuple):
            continue
        bufs, (cap, flags), ((r, region), (rn, regn)) = run
        name, seen = key[1], seen + 1
        assert len(region) == cap and int(r["flags"]) == flags, name
        w = int(r["bytes_written"])
        assert set(region[w:]) <= {0xEE}, name
        near = regn[:int(rn["bytes_written"])]
        if flags & CK:                                                  # the neighbour's header bit and its four checksum bytes
            assert near[4] == neighbour[4] | 4 and len(near) == len(neighbour) + 4
            near = near[:4] + neighbour[4:5] + near[5:-4]
        assert int(rn["status"]) == 0 and near == neighbour and set(regn[int(rn["bytes_written"]):]) <= {0xEE}, name
        if name == "full":
            assert int(r["status"]) == 0 and region == full
        elif name == "full_ck":
            assert int(r["status"]) == 0 and w == cap and region[:4] + region[5:-4] == full[:4] + full[5:] and region[4] == full[4] | 4
        elif name == "full_ck-1":                                       # every block placed, the checksum does not fit
            assert int(r["status"]) == TOO_SMALL and w == len(full) and region[5:w] == full[5:]
            assert int(r["blocks"]) == 3 and int(r["bytes_read"]) == len(bufs[0])
        else:
            k = placed[name]
            assert int(r["status"]) == TOO_SMALL, name
            assert w == (ends[k - 1] if k else (hl if cap >= hl else 0)) and region[:w] == full[:w], (name, w)
            assert int(r["blocks"]) == k and int(r["bytes_read"]) == k * BLOCK, name
    assert seen == 10


def test_bytes_do_not_depend_on_the_batch(runs):
    """A batch mixing one-unit and many-unit frames, forwards and reversed, so that the unit a workgroup had before differs: identical
    frames, and those of the other runs of this file."""
    fwd, rev = frames(runs, "mix"), frames(runs, "mix_reversed")
    assert fwd == rev[::-1]
    constructed = frames(runs, "constructed")
    assert fwd[1] == constructed[1] and fwd[3] == frames(runs, "around")[3]
