"""CZ_COMPRESS_FSE_TABLES (cz_compress_frames_fse_kernel and cz_compress_segments_fse_kernel; czstd_enc.hip, czstd_encsplit.hip and
czstd_encfse.hip unmodified) on the CPU SIMT emulator under ASan + UBSan (tests/emu/emu_encode_fse.cpp), built with one-block
segments (S = 128 KiB) and an 8 KiB overlap.  Every frame must decode to its input under the oracle (status 0, every byte consumed)
and under libzstd where the host has it, stay within cz_compress_bound and leave 0xEE past bytes_written.  The modes and the table
descriptions are read back by tests/compress_fse.py, which shares no code with the kernel.  No GPU needed."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import compress_edges as ce
import compress_frames as cf
import compress_fse as fx
import emu_encode_fse_runner as emu
import oracle
from compress_split import blocks_of

pytestmark = pytest.mark.xdist_group(name="emu_encode_fse")
S, BLOCK = emu.S, 128 << 10
TOO_SMALL = 900
F = emu.FSE_TABLES


def check(name, b, r, region, flags):
    assert int(r["status"]) == 0, name
    n = int(r["bytes_written"])
    frame = region[:n]
    assert n <= emu.compress_bound(len(b)) == len(region), (name, n)
    assert set(region[n:]) <= {0xEE}, f"{name}: bytes past bytes_written were touched"
    assert int(r["bytes_read"]) == len(b) and int(r["blocks"]) == max(1, -(-len(b) // BLOCK)), name
    assert int(r["flags"]) == (flags & (emu.CHECKSUM | F)) | (emu.SPLIT if flags & emu.SPLIT and len(b) > S else 0), name
    st, out, info = oracle.decode_frame(frame, cap=len(b) + 64)
    assert st == 0 and out == b and info["consumed"] == n, (name, st)
    assert info["content_size"] == len(b)
    if flags & emu.CHECKSUM:
        assert info["has_checksum"] and info["checksum"] == oracle.xxh64(b) & 0xFFFFFFFF == int(r["checksum"]), name
    if cf.libzstd():
        assert cf.libzstd_decompress(frame, len(b)) == b, f"{name}: libzstd"
    return frame


@pytest.fixture(scope="module")
def runs():
    """Every emulator run of this file, a few at a time (each is one mostly serial program): name -> (inputs, flags, results)."""
    corpus = [b for _, b in cf.corpus_originals(max_len=6000)]
    special = list(cf.special_inputs().values())
    one, two, fixed, many = fx.one_sequence(), fx.two_sequences(), fx.fixed_copies(), fx.many_ml_codes()
    far = fx.far_offsets()
    jobs = {
        "corpus_on": (corpus, F), "corpus_off": (corpus, 0),
        "modes": ([one, two, fixed, fx.skewed_ml(), fx.gapped_codes(), many, ce.corpus_text(60000)], F),
        "counts": ([far] + [ce.debruijn_tokens(ce.SEQ_LEN[n]) for n in (127, 128, 0x7F00)], F),
        "special_on": (special, F), "special_off": (special, 0),
        "again_1": ([two, fixed], F), "again_2": ([many, one, two, fixed], F | emu.CHECKSUM),
        "split": ([far, fixed, b""], F | emu.SPLIT), "split_checksum": ([far, one], F | emu.SPLIT | emu.CHECKSUM),
    }
    emu.build()
    with ThreadPoolExecutor(4) as ex:
        fut = {k: ex.submit(emu.run, v, flags=fl) for k, (v, fl) in jobs.items()}
        got = {k: (jobs[k][0], jobs[k][1], f.result()) for k, f in fut.items()}
    need = int(got["counts"][2][0][0]["bytes_written"])               # the full frame of `far`: one byte short of it
    got["cap_minus_1"] = ([far, two], F, emu.run([far, two], caps=[need - 1, emu.compress_bound(len(two))], flags=F))
    return got


def frames(runs, key):
    bufs, flags, res = runs[key]
    return [check(f"{key}[{i}]", b, r, region, flags) for i, (b, (r, region)) in enumerate(zip(bufs, res))]


def test_small_corpus_originals(runs):
    """The originals of up to 6 000 bytes with and without the flag: smaller in total, and no frame larger unless its block types
    changed (a Raw block that turns Compressed changes the history of the blocks behind it); at most 2 frames may do that."""
    on, off = frames(runs, "corpus_on"), frames(runs, "corpus_off")
    assert len(on) >= 40
    differ = 0
    for i, (a, b) in enumerate(zip(on, off)):
        if fx.same_block_types(a, b):
            assert len(a) <= len(b), (i, len(a), len(b))
        else:
            differ += 1
    assert differ <= 2
    total_on, total_off = sum(map(len, on)), sum(map(len, off))
    print(f"small corpus originals: {total_on} bytes with the flag, {total_off} without")
    assert total_on < total_off


def test_mode_coverage(runs):
    one, two, fixed, skewed, gapped, many, text = (fx.modes(f) for f in frames(runs, "modes"))
    for m, n in ((one, 1), (two, 2)):                                   # a table cannot pay for itself
        assert len(m) == 1 and m[0]["nseq"] == n and (m[0]["ll"], m[0]["of"], m[0]["ml"]) == (fx.PREDEFINED,) * 3
    (m,) = fixed                                                        # one OF code, one ML code: RLE; LL has two codes: modes mixed
    assert m["nseq"] >= 250 and (m["of"], m["ml"]) == (fx.RLE, fx.RLE) and m["rle"] == {"of": 10, "ml": 39}
    assert m["ll"] != fx.RLE
    (m,) = text
    assert m["nseq"] >= 2000 and (m["ll"], m["of"], m["ml"]) == (fx.FSE,) * 3
    assert (m["tables"]["ll"]["log"], m["tables"]["of"]["log"], m["tables"]["ml"]["log"]) == (9, 8, 9)


def test_table_description_edges(runs):
    bufs, _, _ = runs["modes"]
    fr = frames(runs, "modes")
    # one code at 95 % and more, several codes seen once: "less than 1" probabilities and values in the short form
    (blk,) = [b for b in ce.analyse(fr[3], bufs[3])["blocks"] if b["type"] == "compressed"]
    hist = {}
    for _, ml, _ in blk["seqs"]:
        hist[ce.ml_code(ml)] = hist.get(ce.ml_code(ml), 0) + 1
    assert max(hist.values()) >= 0.95 * len(blk["seqs"]) and sum(1 for c in hist.values() if c == 1) >= 4, hist
    (m,) = fx.modes(fr[3])
    t = m["tables"]["ml"]
    assert m["ml"] == fx.FSE and t["probs"].count(-1) >= 4 and t["short"] >= 1
    assert {s for s, p in enumerate(t["probs"]) if p} == set(hist)
    # used OF codes behind 5 unused codes and 6 apart: chained zero-repeat flags
    (m,) = fx.modes(fr[4])
    t = m["tables"]["of"]
    assert m["of"] == fx.FSE and [s for s, p in enumerate(t["probs"]) if p] == [5, 12] and t["flags"] == [3, 1, 3, 2]
    # more than 32 ML codes in fewer than 256 sequences: the accuracy log is raised to 6
    (m,) = fx.modes(fr[5])
    t = m["tables"]["ml"]
    assert m["ml"] == fx.FSE and m["nseq"] < 256 and sum(1 for p in t["probs"] if p) > 32 and t["log"] == 6
    # offset codes from 17: distances beyond 128 KiB in the second block of an input
    far = frames(runs, "counts")[0]
    m = fx.modes(far)[-1]
    assert m["of"] == fx.FSE and len(m["tables"]["of"]["probs"]) >= 18 and m["tables"]["of"]["probs"][17] > 0


def test_sequence_count_header_forms(runs):
    """127 (one byte), 128 (two) and 0x7F00 (three) sequences in a block, with tables of the block's own."""
    for f, n in zip(frames(runs, "counts")[1:], (127, 128, 0x7F00)):
        (m,) = fx.modes(f)
        assert m["nseq"] == n
        assert fx.FSE in (m["ll"], m["of"], m["ml"])
        (blk,) = ce.parse_frame(f)["blocks"]
        assert blk["seq"]["header_len"] == (1 if n < 128 else (2 if n < 0x7F00 else 3))


def test_special_inputs(runs):
    on, off = frames(runs, "special_on"), frames(runs, "special_off")
    names = list(cf.special_inputs())
    for k in ("empty", "one", "three", "rle64k", "random64k"):          # no sequences: byte for byte as without the flag
        assert on[names.index(k)] == off[names.index(k)], k
    assert all(len(a) <= len(b) for a, b in zip(on, off))


def test_bytes_do_not_depend_on_the_batch(runs):
    """The same buffers at other positions of batches of other sizes and orders (and with the checksum: only the header bit and the
    last four bytes differ)."""
    modes, a1, a2 = frames(runs, "modes"), frames(runs, "again_1"), frames(runs, "again_2")
    one, two, fixed, many = modes[0], modes[1], modes[2], modes[5]
    assert a1 == [two, fixed]
    for with_sum, plain in zip(a2, (many, one, two, fixed)):
        assert with_sum[:4] == plain[:4] and with_sum[4] == plain[4] | 4 and with_sum[5:-4] == plain[5:]


def test_output_too_small_is_a_block_aligned_prefix(runs):
    full, neighbour = frames(runs, "counts")[0], frames(runs, "modes")[1]
    hl, blocks = blocks_of(full)
    assert len(blocks) == 2
    (r, region), (rn, regn) = runs["cap_minus_1"][2]
    assert int(r["status"]) == TOO_SMALL and int(r["flags"]) == F
    w = int(r["bytes_written"])
    assert w == blocks[1][0] and region[:w] == full[:w]                 # the header and the one whole block that fits
    assert int(r["blocks"]) == 1 and int(r["bytes_read"]) == BLOCK
    assert set(region[w:]) <= {0xEE}
    assert int(rn["status"]) == 0 and regn[:int(rn["bytes_written"])] == neighbour and set(regn[len(neighbour):]) <= {0xEE}


def test_split_with_the_flag(runs):
    """One-block segments: segment 0 is the first block of the unsplit flag frame, later segments have tables of their own, inputs
    of at most one segment come out as the unsplit flag frame."""
    far_split, fixed_split, empty = frames(runs, "split")
    far, fixed = frames(runs, "counts")[0], frames(runs, "modes")[2]
    (hs, bs), (hp, bp) = blocks_of(far_split), blocks_of(far)
    assert hs == hp and len(bs) == len(bp) == 2
    assert far_split[:bs[1][0]] == far[:bp[1][0]]
    m = fx.modes(far_split)[-1]                                         # (the far sources are beyond the overlap: fewer OF codes)
    assert m["nseq"] >= 100 and {m["ll"], m["of"], m["ml"]} != {fx.PREDEFINED}
    assert fixed_split == fixed and len(empty) == 9
    assert [int(r["flags"]) for r, _ in runs["split"][2]] == [F | emu.SPLIT, F, F]
    frames(runs, "split_checksum")
    assert [int(r["flags"]) for r, _ in runs["split_checksum"][2]] == [F | emu.SPLIT | emu.CHECKSUM, F | emu.CHECKSUM]
