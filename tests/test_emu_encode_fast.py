"""CZ_COMPRESS_FAST (cz_compress_frames_fast_kernel; the unmodified czstd_encfast.hip) on the CPU SIMT emulator under ASan + UBSan
(tests/emu/emu_encode_fast.cpp).  Every frame must decode to its input under the oracle (status 0, every byte consumed) and under
libzstd where the host has it, stay within cz_compress_bound and leave 0xEE past bytes_written.  The structure of the frames (blocks
of at most 32 KiB that stand alone, Raw groups, repeat offsets) is read back by compress_edges.analyse and compress_split.blocks_of,
which share no code with the kernel.  No GPU needed.

About fx.fixed_copies(): by construction no copy of it has the distance of the copy before it, so no encoder that finds its copies
can write Offset_Value 1 for it (the plain compressor writes none either).  The rule is therefore pinned in both directions for
every Compressed block of every input of this file: Offset_Value 1 stands exactly where a sequence with literals has the actual
offset of the sequence before it in the same block — fixed_copies has no such place, same_distance_copies() has them in every
block — and Offset_Values 2 and 3 never appear."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import compress_edges as ce
import compress_frames as cf
import compress_fse as fx
import emu_encode_fast_runner as emu
import emu_encode_runner as plain
import oracle
from compress_split import blocks_of

pytestmark = pytest.mark.xdist_group(name="emu_encode_fast")
SUB, GROUP, KIB = emu.SUB, emu.GROUP, 1024
TOO_SMALL = 900
F = emu.FAST
LENGTHS = (0, 1, 15, 16, 32 * KIB - 1, 32 * KIB, 32 * KIB + 1, 128 * KIB - 1, 128 * KIB, 128 * KIB + 1, 160 * KIB + 5)
# Block bytes (frames without their headers) of the fast level over those of the plain compressor (flags 0) on the same inputs cut
# into independent 32 KiB pieces, on corpus_text(60000) plus the small corpus originals: measured -0.16 % (60 372 bytes against
# 60 468: the look-back of the fast level covers its whole chunk of 64 positions, which makes up for the smaller table), rounded up
# to the next whole percent.
MAX_EXCESS_PERCENT = 0
SEQ_127, SEQ_128 = 540, 544            # debruijn_tokens lengths that give 127 and 128 sequences (as for the plain compressor)


def random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def raw_groups():
    return random_bytes(128 * KIB + 40000, 11)


def mixed_group():
    """Three sub-blocks of random bytes and one of text: too large for the group to stay below its size only if the text does not compress."""
    return random_bytes(3 * SUB, 12) + ce.corpus_text(SUB)


def period_1000():
    """A pattern of 1 000 bytes without a repeated 4-byte window, laid across the boundary of the first two sub-blocks."""
    p = ce.Gen(13).lit(1000).bytes()
    return (p * 41)[:40000]


def same_distance_copies(n=40000, seed=14):
    """Unique literals with a copy of 64 bytes from 2 000 back every 256 bytes: consecutive sequences with one offset."""
    return ce.mixed(n, seed, every=256, copy=64, dist=2000)


def structure(name, b, frame):
    """The format rules on one frame; returns (blocks_of's list, the analysed blocks)."""
    hl, blocks = blocks_of(frame)
    a = ce.analyse(frame, b)["blocks"]
    assert len(a) == len(blocks)
    for k, ((at, last, btype, size, n), blk) in enumerate(zip(blocks, a)):
        assert last == (k == len(blocks) - 1), name
        start = blk["start"]
        end = a[k + 1]["start"] if k + 1 < len(a) else len(b)
        if btype == 0 and end - start > SUB:                            # a Raw block standing for a whole group
            assert start % GROUP == 0 and end == min(len(b), start + GROUP), (name, k)
            continue
        assert end - start <= SUB and start % SUB == 0, (name, k, start, end)
        if end - start < 16:
            assert btype in (0, 1), (name, k)
        if btype != 2:
            continue
        assert blk["lit"]["type"] in ("raw", "rle", "huffman"), (name, k, blk["lit"]["type"])   # never Treeless
        assert blk["seq"]["modes"] in (0, None), (name, k)              # Predefined three times: never Repeat_Mode
        pos, prev = start, None
        for i, ((ll, ml, ofv), off) in enumerate(zip(blk["seqs"], blk["offsets"])):
            pos += ll
            assert pos - off >= start, f"{name}: block {k} sequence {i} reads in front of its block"
            assert ofv == 1 or ofv > 3, (name, k, i, ofv)
            assert (ofv == 1) == (i > 0 and ll > 0 and off == prev), (name, k, i, ofv, ll, off, prev)
            prev = off
            pos += ml
        if blk["seqs"]:
            assert blk["seqs"][0][2] > 3, (name, k)
    return blocks, a


def check(name, b, r, region, flags):
    assert int(r["status"]) == 0, name
    n = int(r["bytes_written"])
    frame = region[:n]
    assert n <= emu.compress_bound(len(b)) == len(region), (name, n)
    assert set(region[n:]) <= {0xEE}, f"{name}: bytes past bytes_written were touched"
    assert int(r["bytes_read"]) == len(b), name
    assert int(r["flags"]) == flags, name
    st, out, info = oracle.decode_frame(frame, cap=len(b) + 64)
    assert st == 0 and out == b and info["consumed"] == n, (name, st)
    assert info["content_size"] == len(b)
    if flags & emu.CHECKSUM:
        assert info["has_checksum"] and info["checksum"] == oracle.xxh64(b) & 0xFFFFFFFF == int(r["checksum"]), name
    if cf.libzstd():
        assert cf.libzstd_decompress(frame, len(b)) == b, f"{name}: libzstd"
    blocks, _ = structure(name, b, frame)
    assert int(r["blocks"]) == len(blocks), name
    return frame


def pieces(b):
    return [b[i:i + SUB] for i in range(0, len(b), SUB)]


@pytest.fixture(scope="module")
def runs():
    """Every emulator run of this file, a few at a time (each is one mostly serial program): name -> (inputs, flags, results)."""
    text = ce.corpus_text(160 * KIB + 5)
    lengths = [text[:n] for n in LENGTHS]
    corpus = [b for _, b in cf.corpus_originals(max_len=6000)]
    special = list(cf.special_inputs().values())
    t60 = ce.corpus_text(60000)
    fixed, same, per = fx.fixed_copies(), same_distance_copies(), period_1000()
    counts = [ce.debruijn_tokens(SEQ_127), ce.debruijn_tokens(SEQ_128)]
    jobs = {
        "lengths_a": (lengths[:8], F), "lengths_b": (lengths[8:], F),
        "corpus": (corpus, F), "special": (special, F),
        "shapes": ([b"\x07" * 300000, raw_groups(), mixed_group(), per, fixed, same, t60] + counts, F),
        "again_1": ([same, fixed, t60, per], F), "again_2": ([b"x" * 100, per, fixed, lengths[3], t60], F | emu.CHECKSUM),
    }
    yard = {"yard_text": pieces(t60) + pieces(mixed_group()[3 * SUB:]), "yard_corpus": [p for b in corpus for p in pieces(b)]}
    emu.build()
    plain.build()
    with ThreadPoolExecutor(4) as ex:
        fut = {k: ex.submit(emu.run, v, flags=fl) for k, (v, fl) in jobs.items()}
        yfut = {k: ex.submit(plain.run, v, flags=0) for k, v in yard.items()}
        got = {k: (jobs[k][0], jobs[k][1], f.result()) for k, f in fut.items()}
        got.update({k: (yard[k], 0, f.result()) for k, f in yfut.items()})
    two = lengths[-1]                                                   # two groups: one byte short of its full frame
    need = int(got["lengths_b"][2][-1][0]["bytes_written"])
    got["cap_minus_1"] = ([two, per], F, emu.run([two, per], caps=[need - 1, emu.compress_bound(len(per))], flags=F))
    return got


def frames(runs, key):
    bufs, flags, res = runs[key]
    return [check(f"{key}[{i}]", b, r, region, flags) for i, (b, (r, region)) in enumerate(zip(bufs, res))]


def block_bytes(frame):
    hl, blocks = blocks_of(frame)
    return sum(n for *_, n in blocks)


def yard_bytes(runs, key):
    out = []
    for b, (r, region) in zip(runs[key][0], runs[key][2]):
        assert int(r["status"]) == 0
        out.append(block_bytes(region[:int(r["bytes_written"])]))
    return out


def test_boundary_lengths(runs):
    fr = frames(runs, "lengths_a") + frames(runs, "lengths_b")
    for n, f in zip(LENGTHS, fr):
        _, blocks = blocks_of(f)
        assert len(blocks) == max(1, -(-n // SUB)), n                  # text: no group is written Raw
    assert fr[0] == bytes.fromhex("28b52ffd2000010000")                 # the empty input: byte for byte the flags-0 frame
    assert [b[2] for b in blocks_of(fr[2])[1]] == [0]                   # 15 bytes: Raw


def test_special_inputs_and_small_corpus(runs):
    frames(runs, "special")
    fr = frames(runs, "corpus")
    assert len(fr) >= 40
    assert sum(map(len, fr)) < sum(map(len, runs["corpus"][0]))


def test_rle_and_raw_groups(runs):
    fr = frames(runs, "shapes")
    _, blocks = blocks_of(fr[0])                                        # 300 000 equal bytes: every sub-block is RLE
    assert len(blocks) == 10 and {b[2] for b in blocks} == {1} and len(fr[0]) == 9 + 10 * 4
    hl, blocks = blocks_of(fr[1])                                       # random bytes: each group one Raw block
    n = 128 * KIB + 40000
    assert [(b[2], b[3]) for b in blocks] == [(0, GROUP), (0, 40000)] and len(fr[1]) == hl + 2 * 3 + n
    assert int(runs["shapes"][2][1][0]["blocks"]) == 2


def test_mixed_group_keeps_its_blocks(runs):
    """Three Raw blocks and one Compressed: the sum stays below the group's size + 3 (asserted with the plain compressor's size of
    the text piece), so the group is not replaced by one Raw block."""
    text_piece = yard_bytes(runs, "yard_text")[-1]
    assert 3 * (3 + SUB) + text_piece <= GROUP + 3
    _, blocks = blocks_of(frames(runs, "shapes")[2])
    assert [(b[2], b[3]) for b in blocks[:3]] == [(0, SUB)] * 3 and blocks[3][2] == 2 and len(blocks) == 4


def test_blocks_stand_alone_across_a_boundary(runs):
    b = period_1000()
    fr = frames(runs, "shapes")[3]
    blocks, a = structure("period", b, fr)                             # (no source before the block's start: checked there)
    assert len(a) == 2 and a[1]["start"] == SUB and a[1]["type"] == "compressed"
    assert a[1]["seqs"][0][2] > 3
    assert a[1]["lit"]["regen"] >= 1000                                 # the second block pays for the pattern once more


def test_repeat_offsets_in_both_directions(runs):
    fixed, same = frames(runs, "shapes")[4], frames(runs, "shapes")[5]
    for name, b, f, want in (("fixed", fx.fixed_copies(), fixed, False), ("same", same_distance_copies(), same, True)):
        _, a = structure(name, b, f)
        comp = [blk for blk in a if blk["type"] == "compressed"]
        assert len(comp) == 2
        for blk in comp:
            ones = sum(1 for _, _, ofv in blk["seqs"] if ofv == 1)
            assert (ones >= 1) == want, (name, ones)
            if want:
                assert ones >= len(blk["seqs"]) // 2


def test_sequence_count_header_forms(runs):
    for f, n in zip(frames(runs, "shapes")[7:9], (127, 128)):
        (blk,) = ce.parse_frame(f)["blocks"]
        assert blk["seq"]["count"] == n and blk["seq"]["header_len"] == (1 if n < 128 else 2)


def test_bytes_do_not_depend_on_the_batch(runs):
    shapes, a1, a2 = frames(runs, "shapes"), frames(runs, "again_1"), frames(runs, "again_2")
    per, fixed, same, t60 = shapes[3], shapes[4], shapes[5], shapes[6]
    assert a1 == [same, fixed, t60, per]
    sixteen = frames(runs, "lengths_a")[3]
    for with_sum, plain_frame in zip(a2[1:], (per, fixed, sixteen, t60)):
        assert with_sum[:4] == plain_frame[:4] and with_sum[4] == plain_frame[4] | 4 and with_sum[5:-4] == plain_frame[5:]


def test_output_too_small_ends_at_a_group(runs):
    full, neighbour = frames(runs, "lengths_b")[-1], frames(runs, "shapes")[3]
    hl, blocks = blocks_of(full)
    assert len(blocks) == 6
    (r, region), (rn, regn) = runs["cap_minus_1"][2]
    assert int(r["status"]) == TOO_SMALL and int(r["flags"]) == F
    w = int(r["bytes_written"])
    assert w == blocks[4][0] and region[:w] == full[:w]                 # the header and group 0
    assert int(r["blocks"]) == 4 and int(r["bytes_read"]) == GROUP
    assert set(region[w:]) <= {0xEE}
    assert int(rn["status"]) == 0 and regn[:int(rn["bytes_written"])] == neighbour and set(regn[len(neighbour):]) <= {0xEE}


def test_size_against_the_plain_compressor(runs):
    """Not everything Raw: the block bytes stay within MAX_EXCESS_PERCENT of the plain compressor's on independent 32 KiB pieces."""
    t60 = frames(runs, "shapes")[6]
    fast = block_bytes(t60) + sum(map(block_bytes, frames(runs, "corpus")))
    yard = sum(yard_bytes(runs, "yard_text")[:2]) + sum(yard_bytes(runs, "yard_corpus"))
    print(f"fast level: {fast} block bytes, plain compressor on 32 KiB pieces: {yard} ({100.0 * (fast - yard) / yard:.2f} % more)")
    assert fast * 100 <= yard * (100 + MAX_EXCESS_PERCENT)
    a = ce.analyse(t60, ce.corpus_text(60000))["blocks"]
    assert any(blk["type"] == "compressed" and blk["lit"]["type"] == "huffman" and len(blk["seqs"]) >= 100 for blk in a)
