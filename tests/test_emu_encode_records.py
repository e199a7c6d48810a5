"""CZ_COMPRESS_RECORDS (cz_compress_records_kernel and cz_compress_records_dict_kernel; the unmodified czstd_encrec.hip) on the CPU
SIMT emulator under ASan + UBSan (tests/emu/emu_encode_records.cpp).  Without a dictionary every frame and every result field but
`flags` must equal what the fast level gives for the same input (emu_encode_fast_runner).  With dictionaries every frame must decode
to its input under the oracle and, where the host has it, libzstd, each with the dictionary; be one block; stay within
cz_compress_bound; and leave 0xEE past bytes_written.  That the dictionary is used, and each branch of the dictionary path, is read
back by compress_edges.analyse, which shares no code with the kernel.  No GPU needed."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import compress_edges as ce
import compress_frames as cf
import dict_build as db
import dict_edges as de
import dict_frames as dfr
import dict_records as dr
import emu_encode_dict_runner as olddict
import emu_encode_fast_runner as fast
import emu_encode_records_runner as emu
import oracle
import records_edges as rede
from compress_split import blocks_of

pytestmark = pytest.mark.xdist_group(name="emu_encode_records")
KIB, MAXREC = 1024, emu.RECORD_MAX
R, CK, NOID, NO_DICT = emu.RECORDS, emu.CHECKSUM, emu.NO_DICT_ID, emu.NO_DICT
INVALID_ARG, TOO_SMALL = 901, 900
LENGTHS = (0, 1, 15, 16, 17, 255, 256, 32 * KIB - 1, 32 * KIB)
LIT_UNDER, LIT_OVER = 6724, 6725        # prefixes of corpus_text whose block has 1 023 and 1 024 literals (asserted below)
FIELDS = ("status", "blocks", "bytes_read", "bytes_written", "checksum")
# Total frame bytes of dict_records.records(200) with their dictionaries at this level over those of the dictionary compressor
# (flags 0, emu_encode_dict_runner) on the same records, on the emulator: measured -0.81 % (69 673 bytes against 70 244: the
# look-back over the whole chunk and the chunk-wide parse make up for the 12-bit table and for the dictionary's repeat offsets,
# which this level does not use), rounded up to the next whole percent.
MAX_EXCESS_PERCENT = 0


def text():
    return ce.corpus_text(32 * KIB + 1)


def nodict_inputs():
    t = text()
    special = [b for _, b in sorted(cf.special_inputs().items()) if len(b) <= MAXREC]
    corpus = [b for _, b in cf.corpus_originals(max_len=MAXREC)]
    return [t[:n] for n in LENGTHS] + [t[:LIT_UNDER], t[:LIT_OVER]] + special + corpus


@pytest.fixture(scope="module")
def nodict():
    """{flags: results} of the records level (64, 65) and the fast level (32, 33) on the same inputs, and the oversize record."""
    bufs = nodict_inputs()
    emu.build()
    fast.build()
    with ThreadPoolExecutor(4) as ex:
        fut = {R: ex.submit(emu.run, bufs, flags=R), R | CK: ex.submit(emu.run, bufs, flags=R | CK),
               fast.FAST: ex.submit(fast.run, bufs, flags=fast.FAST), fast.FAST | CK: ex.submit(fast.run, bufs, flags=fast.FAST | CK)}
        got = {k: f.result() for k, f in fut.items()}
    got["bufs"] = bufs
    return got


@pytest.fixture(scope="module")
def family():
    """dict_records.records(25, seed=99) with the four family dictionaries: {flags: results} for 64, 65, 66 and 67."""
    recs = dr.records(25, seed=99)
    bufs, idx, dicts = [b for _, b in recs], [j for j, _ in recs], dr.dictionaries()
    emu.build()
    with ThreadPoolExecutor(4) as ex:
        fut = {fl: ex.submit(emu.run, bufs, dicts, idx, flags=fl) for fl in (R, R | CK, R | NOID, R | CK | NOID)}
        got = {k: f.result() for k, f in fut.items()}
    got.update(bufs=bufs, idx=idx, dicts=dicts)
    return got


def decodes_with(frame, b, dictionary, dname=None):
    st, out = oracle.decode_frame_with_dict(frame, oracle.Dictionary(dictionary), cap=len(b) + 64)
    assert st == 0 and out == b, st
    if dr.libzstd():
        got = dr.zstd_decompress_dict(frame, len(b), dictionary)
        if dname in db.LIBZSTD_REFUSES:
            assert got is None, "libzstd was expected to refuse the dictionary"
        else:
            assert got == b, "libzstd"


def check_region(name, b, r, region, flags):
    """status 0, the flags (as in the plain dictionary calls the result does not repeat CZ_COMPRESS_NO_DICT_ID), the whole input
    read, one block, within the bound, nothing past bytes_written; returns the frame."""
    assert int(r["status"]) == 0 and int(r["flags"]) == flags & ~NOID, (name, r)
    n = int(r["bytes_written"])
    assert n <= emu.compress_bound(len(b)) == len(region), (name, n)
    assert set(region[n:]) <= {0xEE}, f"{name}: bytes past bytes_written were touched"
    assert int(r["bytes_read"]) == len(b) and int(r["blocks"]) == 1, name
    frame = region[:n]
    hl, blocks = blocks_of(frame)
    assert len(blocks) == 1 and blocks[0][1], name                     # one block, the last
    if len(b) < 16:
        assert blocks[0][2] in (0, 1), name
    if flags & CK:
        assert int.from_bytes(frame[-4:], "little") == oracle.xxh64(b) & 0xFFFFFFFF == int(r["checksum"]) and frame[4] & 4, name
    else:
        assert not frame[4] & 4, name
    return frame


# ------------------------------------------------------------------------------------------------ 1. no dictionary = the fast level
def test_without_a_dictionary_the_frames_are_the_fast_levels(nodict):
    bufs = nodict["bufs"]
    assert len(bufs) >= len(LENGTHS) + 2 + 5 + 40
    for rf, ff in ((R, fast.FAST), (R | CK, fast.FAST | CK)):
        for i, (b, (r, region), (r2, region2)) in enumerate(zip(bufs, nodict[rf], nodict[ff])):
            assert region == region2, (rf, i, len(b))
            assert all(int(r[k]) == int(r2[k]) for k in FIELDS), (rf, i, r, r2)
            assert int(r["flags"]) == rf and int(r2["flags"]) == ff
            frame = check_region(f"nodict[{i}]", b, r, region, rf)
            st, out, info = oracle.decode_frame(frame, cap=len(b) + 64)
            assert st == 0 and out == b and info["consumed"] == len(frame), (i, st)
    assert nodict[R][0][1][:9] == bytes.fromhex("28b52ffd2000010000")     # the empty input: one empty last Raw block


def test_one_and_four_streams_around_1_kib_of_literals(nodict):
    bufs = nodict["bufs"]
    for n, streams in ((LIT_UNDER, 1), (LIT_OVER, 4)):
        i = next(k for k, b in enumerate(bufs) if len(b) == n)
        r, region = nodict[R][i]
        (blk,) = ce.analyse(region[:int(r["bytes_written"])], bufs[i])["blocks"]
        assert blk["lit"]["type"] == "huffman" and blk["lit"]["streams"] == streams, blk["lit"]
        assert (blk["lit"]["regen"] == 1023) if streams == 1 else (blk["lit"]["regen"] == 1024), blk["lit"]["regen"]


def test_a_record_above_the_limit_fails_alone():
    t = text()
    for dicts, idx in ((None, None), (dr.dictionaries()[:1], [0, 0, NO_DICT])):
        bufs = [t[:200], t[:MAXREC + 1], t[:MAXREC + 1] if dicts else t[:300]]
        got = emu.run(bufs, dicts, idx, flags=R)
        (r0, g0), (r1, g1), (r2, g2) = got
        assert int(r0["status"]) == 0
        for r, g in ((r1, g1),) + (((r2, g2),) if dicts else ()):
            assert (int(r["status"]), int(r["blocks"]), int(r["bytes_read"]), int(r["bytes_written"]), int(r["flags"])) == (INVALID_ARG, 0, 0, 0, R)
            assert set(g) == {0xEE}
        if not dicts:
            assert int(r2["status"]) == 0


# ---------------------------------------------------------------------------------------------- 2. dictionaries: decoding, headers
def test_dictionary_frames_decode_and_are_one_block(family):
    bufs, idx, dicts = family["bufs"], family["idx"], family["dicts"]
    ids = [oracle.Dictionary(d).info["id"] for d in dicts]
    for flags in (R, R | CK, R | NOID, R | CK | NOID):
        for i, (b, j, (r, region)) in enumerate(zip(bufs, idx, family[flags])):
            frame = check_region(f"family[{i}]", b, r, region, flags)
            decodes_with(frame, b, dicts[j])
            width, did = dfr.header_id(frame)
            if flags & NOID:
                assert width == 0, i
            else:
                assert did == ids[j] and width == (1 if did < 256 else (2 if did < 65536 else 4)), (i, width, did)
    for (r, a), (r2, a2) in zip(family[R], family[R | CK]):              # the checksum changes the flag bit and the last four bytes
        n, n2 = int(r["bytes_written"]), int(r2["bytes_written"])
        assert n2 == n + 4 and a2[:4] == a[:4] and a2[4] == a[4] | 4 and a2[5:n] == a[5:n]
    for (r, a), (r2, a2) in zip(family[R], family[R | NOID]):           # ... and the ID only the header
        n, n2 = int(r["bytes_written"]), int(r2["bytes_written"])
        w = dfr.header_id(a)[0]
        assert n2 == n - w and a2[5:n2] == a[5 + w:n] and a2[4] == a[4] & ~3


# ------------------------------------------------------------------------------------- 3. dictionaries: the dictionary is really used
def test_the_dictionary_is_really_used(family):
    bufs, idx, dicts = family["bufs"], family["idx"], family["dicts"]
    treeless = repeat = inside = 0
    for b, j, (r, region) in zip(bufs, idx, family[R]):
        (blk,) = ce.analyse(region[:int(r["bytes_written"])], b, dictionary=dicts[j])["blocks"]
        if blk["type"] != "compressed":
            continue
        treeless += blk["lit"]["type"] == "treeless"
        repeat += bool(blk["seqs"]) and de.modes(blk) == (3, 3, 3)
        pos = 0
        for (ll, ml, _), off in zip(blk["seqs"], blk["offsets"]):
            pos += ll
            inside += off > pos                                         # the source lies in front of the input: in the content
            pos += ml
    assert treeless >= 1 and repeat >= 1 and inside >= 1, (treeless, repeat, inside)
    assert treeless >= 50 and inside >= 100                             # (these records are what the dictionaries were made for)


# ------------------------------------------------------------------------------------------------ 4. edges of the dictionary path
@pytest.fixture(scope="module")
def edge_runs():
    E = rede.edges()
    bufs, dicts, idx = de.batch(E)
    return E, emu.run(bufs, dicts, idx, flags=R | CK)


def test_edges_decode_and_reach_their_branches(edge_runs):
    E, got = edge_runs
    for e, (r, region) in zip(E, got):
        frame = check_region(e.name, e.data, r, region, R | CK)
        try:
            decodes_with(frame, e.data, e.dictionary, e.dname)
            fr = ce.analyse(frame, e.data, dictionary=e.dictionary)
            e.check(fr)
            de.check_header(e, frame)
        except AssertionError as ex:
            raise AssertionError(f"{e.name} misses its branch: {ex}") from ex
        for b in fr["blocks"]:
            if b["type"] == "compressed":
                assert all(o <= ce.WINDOW for o in b["offsets"]), e.name
                prev = None
                for i, ((ll, _, ofv), off) in enumerate(zip(b["seqs"], b["offsets"])):   # the repeat rule, in both directions
                    assert (ofv == 1) == (i > 0 and ll > 0 and off == prev) and (ofv == 1 or ofv > 3), (e.name, i, ofv)
                    prev = off


# ------------------------------------------------------------------------------------- 5. scheduling cannot show in the bytes
def test_scheduling_cannot_show_in_the_bytes(family):
    bufs, idx, dicts = family["bufs"][:9], family["idx"][:9], family["dicts"]
    want = [region[:int(r["bytes_written"])] for r, region in family[R][:9]]

    def frames(b, ix):
        got = emu.run(b, dicts, ix, flags=R)
        for r, region in got:
            assert int(r["status"]) == 0 and int(r["flags"]) == R and int(r["blocks"]) == 1, r      # no 0xA5 left in any record
        return [region[:int(r["bytes_written"])] for r, region in got]
    with ThreadPoolExecutor(4) as ex:
        parts = {n: ex.submit(lambda n=n: [f for k in range(0, 9, n) for f in frames(bufs[k:k + n], idx[k:k + n])]) for n in (1, 4, 5)}
        rev = ex.submit(frames, bufs[::-1], idx[::-1])
        mixed_b = [x for b in bufs for x in (b, b)]
        mixed_i = [x for j in idx for x in (j, NO_DICT)]
        mix = ex.submit(frames, mixed_b, mixed_i)
        plain = ex.submit(emu.run, bufs, None, None, None, R)
        for n, f in parts.items():
            assert f.result() == want, n
        assert rev.result()[::-1] == want
        assert mix.result()[0::2] == want
        assert mix.result()[1::2] == [region[:int(r["bytes_written"])] for r, region in plain.result()]   # NO_DICT: the plain kernel's frame


# ------------------------------------------------------------------------------------------------ 6. mixed failures in one batch
def test_mixed_failures_in_one_batch(family):
    bufs, dicts = family["bufs"], family["dicts"]
    good, nod, tight = bufs[0], bufs[1], bufs[4]                        # (0 and 4: the first family; 1: written without a dictionary)
    big = text()[:MAXREC + 1]
    clean = emu.run([good, nod, tight], dicts, [0, NO_DICT, 0], flags=R | CK)
    need = int(clean[2][0]["bytes_written"])
    batch = [good, good, big, nod, tight]
    caps = [emu.compress_bound(len(b)) for b in batch[:4]] + [need - 1]
    got = emu.run(batch, dicts, [0, 4, 0, NO_DICT, 0], caps=caps, flags=R | CK)
    for k in (1, 2):                                                    # the bad index, the oversize record
        r, region = got[k]
        assert (int(r["status"]), int(r["blocks"]), int(r["bytes_read"]), int(r["bytes_written"]), int(r["flags"])) == (INVALID_ARG, 0, 0, 0, R | CK), k
        assert set(region) == {0xEE}, k
    for k, c in ((0, 0), (3, 1)):
        (r, region), (rc, regc) = got[k], clean[c]
        assert int(r["status"]) == 0 and region == regc and all(int(r[f]) == int(rc[f]) for f in FIELDS), k
    r, region = got[4]
    w = int(r["bytes_written"])
    assert int(r["status"]) == TOO_SMALL and int(r["flags"]) == R | CK and len(region) == need - 1
    assert w <= need - 1 and region[:w] == clean[2][1][:w] and set(region[w:]) <= {0xEE}
    assert w == need - 4 and int(r["blocks"]) == 1                      # header and block fit; the checksum does not


# ------------------------------------------------------------------------------------------------------------- 7. size yardstick
def test_size_against_the_dictionary_compressor():
    """Not everything Raw: the frame bytes stay within MAX_EXCESS_PERCENT of the existing dictionary compressor's."""
    recs = dr.records(200)
    bufs, idx, dicts = [b for _, b in recs], [j for j, _ in recs], dr.dictionaries()
    olddict.build()
    with ThreadPoolExecutor(2) as ex:
        a, b = ex.submit(emu.run, bufs, dicts, idx, flags=R), ex.submit(olddict.run, bufs, dicts, index=idx, flags=0)
        new, old = a.result(), b.result()
    assert all(int(r["status"]) == 0 for r, _ in new + old)
    n, o = sum(int(r["bytes_written"]) for r, _ in new), sum(int(r["bytes_written"]) for r, _ in old)
    print(f"records level: {n} frame bytes, dictionary compressor: {o} ({100.0 * (n - o) / o:.2f} % more), input {sum(map(len, bufs))}")
    assert n * 100 <= o * (100 + MAX_EXCESS_PERCENT)
