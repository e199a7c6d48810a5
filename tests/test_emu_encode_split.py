"""CZ_COMPRESS_SPLIT (cz_compress_plan_kernel and cz_compress_segments_kernel, czstd_enc.hip and czstd_encsplit.hip unmodified) on
the CPU SIMT emulator under ASan + UBSan (tests/emu/emu_encode_split.cpp), built with one-block segments (S = 128 KiB) and an
8 KiB overlap.  The emulator runs workgroups one after another, so this checks the frame format and the chain bookkeeping, not
concurrency (tests/test_compress_split_gpu.py does that).  Every frame must decode to its input under the oracle (status 0, every
byte consumed, content size) and under libzstd where the host has it, stay within cz_compress_bound and leave 0xEE past
bytes_written.  No GPU needed."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import compress_frames as cf
import emu_encode_runner as plain_emu
import emu_encode_split_runner as emu
import oracle
from compress_split import blocks_of, first_offset_code, text

pytestmark = pytest.mark.xdist_group(name="emu_encode_split")
S, BLOCK = emu.S, 128 << 10
TOO_SMALL = 900


def check(name, b, r, region, flags):
    assert int(r["status"]) == 0, name
    n = int(r["bytes_written"])
    frame = region[:n]
    assert n <= emu.compress_bound(len(b)) == len(region), (name, n)
    assert set(region[n:]) <= {0xEE}, f"{name}: bytes past bytes_written were touched"
    assert int(r["bytes_read"]) == len(b) and int(r["blocks"]) == max(1, -(-len(b) // BLOCK)), name
    assert int(r["flags"]) == (flags & emu.CHECKSUM) | (emu.SPLIT if len(b) > S else 0), name
    st, out, info = oracle.decode_frame(frame, cap=len(b) + 64)
    assert st == 0 and out == b and info["consumed"] == n, (name, st)
    assert info["content_size"] == len(b)
    if flags & emu.CHECKSUM:
        assert info["has_checksum"] and info["checksum"] == oracle.xxh64(b) & 0xFFFFFFFF, name
        assert int(r["checksum"]) == oracle.xxh64(b) & 0xFFFFFFFF
    if cf.libzstd():
        assert cf.libzstd_decompress(frame, len(b)) == b, f"{name}: libzstd"
    hl, blocks = blocks_of(frame)
    assert [last for _, last, _, _, _ in blocks] == [0] * (len(blocks) - 1) + [1], name
    assert len(blocks) == int(r["blocks"])
    return frame


@pytest.fixture(scope="module")
def runs():
    """Every emulator run of this file, a few at a time (each is one mostly serial program): name -> (inputs, results)."""
    rng = np.random.default_rng(99)
    T = text(2 * S + 70001)
    period = bytearray(rng.bytes(1000) * (2 * S // 1000 + 6))[:2 * S + 5000]
    for k in (1, 2):                                                    # a byte that breaks the period right behind each cut:
        period[k * S + 2] ^= 0x55                                       # the segment's first sequence then has literals
    period = bytes(period)
    capin = b"\0" * S + text(S, skip=777) + text(5000, skip=31)         # 3 segments: an RLE block, a Compressed one, a short tail
    small = text(3000, skip=5)
    inputs = {
        "short": [b"", b"\x41", T[:S - 1], T[:S]],
        "text": [T[:S + 1], T[:2 * S], T],
        "special": [b"\0" * (3 * S), rng.bytes(2 * S), rng.bytes(S) + text(40000, skip=123), period],
        "checksum": [T[:S + 1], capin, b"", small],
        "cap_full": [capin, small],
    }
    plain_inputs = {
        "short": inputs["short"], "text": inputs["text"],
        "pieces": [T[S:S + 1], T[S:2 * S], T[2 * S:]],                  # (T[:S] is in "short")
        "period": [period],
    }
    jobs = {("split", k): (emu.run, v, dict(flags=emu.SPLIT | (emu.CHECKSUM if k == "checksum" else 0))) for k, v in inputs.items()}
    jobs.update({("plain", k): (plain_emu.run, v, dict(flags=0)) for k, v in plain_inputs.items()})
    emu.build(), plain_emu.build()
    with ThreadPoolExecutor(4) as ex:
        fut = {k: ex.submit(fn, v, **kw) for k, (fn, v, kw) in jobs.items()}
        got = {k: (jobs[k][1], f.result()) for k, f in fut.items()}
    # the two out_cap runs need the full frame's layout first
    full = got[("split", "cap_full")][1][0]
    need = int(full[0]["bytes_written"])
    hl, blocks = blocks_of(full[1][:need])
    caps = {"cap_minus_1": need - 1, "cap_in_seg1": blocks[1][0] + blocks[1][4] // 2}
    with ThreadPoolExecutor(2) as ex:
        fut = {k: ex.submit(emu.run, [capin, small], caps=[c, emu.compress_bound(len(small))], flags=emu.SPLIT) for k, c in caps.items()}
        for k, f in fut.items():
            got[("split", k)] = ([capin, small], f.result())
    return got


def frames(runs, kind, key, flags=0):
    bufs, res = runs[(kind, key)]
    if kind == "plain":
        return [region[:int(r["bytes_written"])] for r, region in res]
    return [check(f"{key}[{i}]", b, r, region, flags) for i, (b, (r, region)) in enumerate(zip(bufs, res))]


def test_up_to_one_segment_is_the_plain_frame(runs):
    """Lengths 0, 1, S - 1 and S: byte for byte the frames of cz_compress_frames_kernel, flags without SPLIT."""
    split = frames(runs, "split", "short")
    assert split == frames(runs, "plain", "short")
    assert all(int(r["flags"]) == 0 for r, _ in runs[("split", "short")][1])


def test_split_text_frames(runs):
    """S + 1, 2 S and 2 S + 70 001 bytes of corpus text: one block per 128 KiB, Last_Block on the final one only (check), the first
    segment byte for byte the plain frame's, and the frame no larger than the plain frames of its segments together."""
    split, plain = frames(runs, "split", "text"), frames(runs, "plain", "text")
    piece = {0: frames(runs, "plain", "short")[3]}                      # T[:S]
    piece[(1, 1)], piece[(1, S)], piece[(2, 70001)] = frames(runs, "plain", "pieces")
    for b, fs, fp in zip(runs[("split", "text")][0], split, plain):
        hl, blocks = blocks_of(fs)
        assert len(blocks) == -(-len(b) // BLOCK)
        seg0 = blocks[0][0] + blocks[0][4]                              # header and the one block of segment 0
        assert hl == blocks_of(fp)[0] and fs[:seg0] == fp[:seg0]
        pieces = [piece[0], piece[(1, min(len(b) - S, S))]] + ([piece[(2, 70001)]] if len(b) > 2 * S else [])
        assert len(fs) <= sum(map(len, pieces)), (len(b), len(fs), [len(p) for p in pieces])
        assert int(runs[("split", "text")][1][0][0]["flags"]) == emu.SPLIT


def test_rle_raw_and_history_behind_raw(runs):
    zeros, rnd, rnd_text, _ = frames(runs, "split", "special")
    assert [t for t, _ in cf.walk(zeros)] == ["rle"] * 3
    assert [t for t, _ in cf.walk(rnd)] == ["raw"] * 2
    # a Raw segment 0, then text: the later segment starts from a history of its own whatever segment 0 wrote
    assert [t for t, _ in cf.walk(rnd_text)] == ["raw", "compressed"]


def test_first_offset_of_a_segment_is_explicit(runs):
    """A 1 000-byte period over 3 segments, broken by one byte right behind each cut: the first sequence of every later segment has
    literals and repeats the offset the segment before ended with.  The unsplit frame writes it as Offset_Value 1 (code 0); a split
    frame must write it explicitly (1 000 + 3: code 9), since the segment cannot know the decoder's history."""
    fs = frames(runs, "split", "special")[3]
    fp = frames(runs, "plain", "period")[0]
    (_, bs), (_, bp) = blocks_of(fs), blocks_of(fp)
    assert [b[2] for b in bs] == [2, 2, 2] == [b[2] for b in bp]
    assert fs[:bs[1][0]] == fp[:bp[1][0]]
    for k in (1, 2):
        assert first_offset_code(fp[bp[k][0]:bp[k][0] + bp[k][4]]) == 0
        assert first_offset_code(fs[bs[k][0]:bs[k][0] + bs[k][4]]) == 9
    assert first_offset_code(fs[bs[0][0]:bs[0][0] + bs[0][4]]) == 9    # the period's first match: explicit in both
    assert len(fs) < 1000 + 200                                         # every segment found the period across its cut


def test_checksum(runs):
    """The checksum of a split frame comes from its checksum unit, that of a short one from its own workgroup."""
    frames(runs, "split", "checksum", flags=emu.CHECKSUM)
    assert [int(r["flags"]) for r, _ in runs[("split", "checksum")][1]] == [emu.SPLIT | emu.CHECKSUM] * 2 + [emu.CHECKSUM] * 2


@pytest.mark.parametrize("which,placed", [("cap_minus_1", 2), ("cap_in_seg1", 1)])
def test_output_too_small_is_a_block_aligned_prefix(runs, which, placed):
    full, neighbour = frames(runs, "split", "cap_full")
    hl, blocks = blocks_of(full)
    (r, region), (rn, regn) = runs[("split", which)][1]
    assert int(r["status"]) == TOO_SMALL
    w = int(r["bytes_written"])
    assert w == blocks[placed][0] and region[:w] == full[:w]            # header and the whole blocks placed
    assert int(r["blocks"]) == placed and int(r["bytes_read"]) == placed * BLOCK
    assert set(region[w:]) <= {0xEE}
    assert int(r["flags"]) == emu.SPLIT
    assert int(rn["status"]) == 0 and regn[:int(rn["bytes_written"])] == neighbour and set(regn[len(neighbour):]) <= {0xEE}
