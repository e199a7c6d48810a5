"""CZ_COMPRESS_FAST_SPLIT (cz_compress_fast_plan_kernel, cz_compress_groups_fast_kernel; the unmodified czstd_encfastsplit.hip) on the
CPU SIMT emulator under ASan + UBSan (tests/emu/emu_encode_fast_split.cpp).  The specification is an equality: for every input, every
out_cap and both checksum settings the frame and the result fields status, blocks, bytes_read, bytes_written and checksum are those of
the fast level (tests/emu/emu_encode_fast.cpp, run here on the same batch), and `flags` carries 128 where the fast frame carries 32.
What the fast level's frames look like is checked in test_emu_encode_fast.py.  The emulator runs workgroups one after another, so
this checks the plan, the unit search and the chain bookkeeping, not concurrency.  No GPU needed."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import compress_edges as ce
import compress_frames as cf
import emu_encode_fast_runner as fast
import emu_encode_fast_split_runner as emu
import oracle
from compress_split import blocks_of
from test_emu_encode_fast import mixed_group, random_bytes, raw_groups

pytestmark = pytest.mark.xdist_group(name="emu_encode_fast_split")
SUB, GROUP, KIB = emu.SUB, emu.GROUP, 1024
OK, TOO_SMALL = 0, 900
FS, F, CKS = emu.FAST_SPLIT, fast.FAST, emu.CHECKSUM
LENGTHS = (0, 1, 15, 16, 32 * KIB - 1, 32 * KIB, 32 * KIB + 1, 128 * KIB - 1, 128 * KIB, 128 * KIB + 1, 160 * KIB + 5, 256 * KIB + 5)
FIELDS = ("status", "blocks", "bytes_read", "bytes_written", "checksum")


def three_groups():
    """Three groups whose block counts differ from their group counts: a sub-block of text and three of zeros (one Compressed and
    three RLE blocks), 128 KiB of random bytes (ONE Raw block for the group), 5 000 bytes of text (one block)."""
    return ce.corpus_text(SUB) + bytes(3 * SUB) + random_bytes(GROUP, 21) + ce.corpus_text(SUB + 5000)[SUB:]


def two_groups():
    return ce.corpus_text(2 * SUB)[SUB:] + bytes(3 * SUB) + ce.corpus_text(100)


def same(name, got, want, cks):
    """The records and regions of a fast-split run against those of the fast level's run of the same batch and caps."""
    assert len(got) == len(want)
    for i, ((r, region), (q, wanted)) in enumerate(zip(got, want)):
        for k in FIELDS:
            assert int(r[k]) == int(q[k]), (name, i, k, int(r[k]), int(q[k]))
        assert int(r["flags"]) == FS | cks and int(q["flags"]) == F | cks, (name, i, int(r["flags"]))
        assert region == wanted, f"{name}[{i}]: the output region differs from the fast level's"
        assert set(region[int(r["bytes_written"]):]) <= {0xEE}, f"{name}[{i}]: bytes past bytes_written were touched"


@pytest.fixture(scope="module")
def runs():
    """Every emulator run of this file, a few at a time: name -> (inputs, caps, checksum bit, fast-split results, fast results)."""
    text = ce.corpus_text(max(LENGTHS))
    lengths = [text[:n] for n in LENGTHS]
    three, two = three_groups(), two_groups()
    batches = {
        "lengths_a": lengths[:9], "lengths_b": lengths[9:],
        "shapes": [raw_groups(), mixed_group(), b"\x07" * 300000, three],
    }
    mixed = [text[:1], three, text[:SUB + 1], two, b""]                 # one unit, three (+ a checksum unit), one, two, one
    emu.build()
    fast.build()
    got = {}
    with ThreadPoolExecutor(4) as ex:
        fut = {}
        for key, bufs in batches.items():
            for cks in (0, CKS):
                fut[key, cks] = (ex.submit(emu.run, bufs, flags=FS | cks), ex.submit(fast.run, bufs, flags=F | cks))
        for cks in (0, CKS):
            fut["mixed", cks] = (ex.submit(emu.run, mixed, flags=FS | cks), ex.submit(fast.run, mixed, flags=F | cks))
            fut["mixed_reversed", cks] = (ex.submit(emu.run, mixed[::-1], flags=FS | cks), None)
        for (key, cks), (a, b) in fut.items():
            bufs = batches.get(key, mixed[::-1] if key == "mixed_reversed" else mixed)
            got[key, cks] = (bufs, None, cks, a.result(), b.result() if b else None)
        # the out_cap sweep on the three-group input, from the block list of its full fast frame
        sweeps = {}
        for cks in (0, CKS):
            r, region = got["shapes", cks][4][3]
            full = int(r["bytes_written"])
            hl, blocks = blocks_of(region[:full])
            assert [b[2] for b in blocks] == [2, 1, 1, 1, 0, 2], blocks      # Compressed, 3 x RLE | one Raw group | Compressed
            ends = [blocks[4][0], blocks[5][0], blocks[5][0] + blocks[5][4]]   # where groups 0, 1 and 2 end
            assert ends[2] + (4 if cks else 0) == full
            caps = [hl - 1, hl] + [e - d for e in ends for d in (1, 0)] + ([full - 1, full] if cks else [])
            sweeps[cks] = (caps, hl, ends, full)
            bufs = [three] * len(caps)
            fut["sweep", cks] = (ex.submit(emu.run, bufs, caps=caps, flags=FS | cks), ex.submit(fast.run, bufs, caps=caps, flags=F | cks))
        for cks in (0, CKS):
            a, b = fut["sweep", cks]
            got["sweep", cks] = ([three] * len(sweeps[cks][0]), sweeps[cks], cks, a.result(), b.result())
    return got


@pytest.mark.parametrize("cks", (0, CKS))
@pytest.mark.parametrize("key", ("lengths_a", "lengths_b", "shapes"))
def test_frames_and_records_equal_the_fast_level(runs, key, cks):
    bufs, _, _, got, want = runs[key, cks]
    same(key, got, want, cks)
    for b, (r, region) in zip(bufs, got):
        assert int(r["status"]) == OK and int(r["bytes_read"]) == len(b)
        assert int(r["bytes_written"]) <= emu.compress_bound(len(b)) == len(region)


def test_block_counts_do_not_count_groups(runs):
    """Two Raw groups are two blocks, the mixed group four, 300 000 equal bytes ten RLE blocks in three groups, and the three-group
    input 4 + 1 + 1: a successor cannot tell the groups placed from the blocks placed."""
    got = runs["shapes", 0][3]
    assert [int(r["blocks"]) for r, _ in got] == [2, 4, 10, 6]
    (r, region) = got[0]
    assert [(b[2], b[3]) for b in blocks_of(region[:int(r["bytes_written"])])[1]] == [(0, GROUP), (0, 40000)]


@pytest.mark.parametrize("cks", (0, CKS))
def test_out_cap_sweep(runs, cks):
    """header - 1, header, the end of each group - 1 and exact, and with the checksum full - 1 (the 4 bytes do not fit) and full:
    every field and every byte of the region as from the fast level at the same cap, CZ_E_OUTPUT_TOO_SMALL in its three places."""
    _, (caps, hl, ends, full), _, got, want = runs["sweep", cks]
    same("sweep", got, want, cks)
    rec = [tuple(int(r[k]) for k in ("status", "blocks", "bytes_read", "bytes_written")) for r, _ in got]
    n = 2 * GROUP + 5000
    assert rec[0] == (TOO_SMALL, 0, 0, 0)                               # the header does not fit
    assert rec[1] == (TOO_SMALL, 0, 0, hl) and rec[2] == rec[1][:3] + (hl,)   # group 0 does not fit: the header alone
    assert rec[3] == rec[4] == (TOO_SMALL, 4, GROUP, ends[0])           # the frame ends behind group 0
    assert rec[5] == rec[6] == (TOO_SMALL, 5, 2 * GROUP, ends[1])
    if not cks:
        assert rec[7] == (OK, 6, n, full) and len(rec) == 8
    else:
        assert rec[7] == rec[8] == (TOO_SMALL, 6, n, ends[2])           # every block placed, the checksum bytes do not fit
        assert rec[9] == (OK, 6, n, full) and len(rec) == 10
        assert int(got[7][0]["checksum"]) == int(got[9][0]["checksum"]) == oracle.xxh64(three_groups()) & 0xFFFFFFFF
    assert all(int(r["checksum"]) == 0 for r, _ in got[:7])


@pytest.mark.parametrize("cks", (0, CKS))
def test_bytes_do_not_depend_on_the_batch(runs, cks):
    """One-unit and many-unit frames in one batch, forwards and reversed: the same frame per input, and the fast level's."""
    bufs, _, _, fwd, want = runs["mixed", cks]
    same("mixed", fwd, want, cks)
    rev = runs["mixed_reversed", cks][3][::-1]
    same("mixed_reversed", rev, want, cks)
    three = runs["shapes", cks][3][3]
    assert fwd[1][1] == three[1] and int(fwd[1][0]["blocks"]) == int(three[0]["blocks"]) == 6
    assert [int(r["blocks"]) for r, _ in fwd] == [1, 6, 2, 5, 1]


def test_one_frame_of_each_kind_decodes(runs):
    for key, i, cks in (("mixed", 1, 0), ("mixed", 1, CKS), ("mixed", 3, CKS), ("mixed", 4, CKS), ("mixed", 0, 0), ("shapes", 0, CKS),
                        ("shapes", 1, 0), ("shapes", 2, CKS), ("lengths_b", 2, CKS)):
        b = runs[key, cks][0][i]
        r, region = runs[key, cks][3][i]
        frame = region[:int(r["bytes_written"])]
        st, out, info = oracle.decode_frame(frame, cap=len(b) + 64)
        assert st == 0 and out == b and info["consumed"] == len(frame), (key, i, cks, st)
        assert info["content_size"] == len(b)
        if cks:
            assert info["has_checksum"] and info["checksum"] == oracle.xxh64(b) & 0xFFFFFFFF == int(r["checksum"]), (key, i)
        if cf.libzstd():
            assert cf.libzstd_decompress(frame, len(b)) == b, f"{key}[{i}]: libzstd"
