"""tests/dict_build.py, the writer of the hand-built dictionaries of tests/dict_edges.py, against three readers that share no code
with it or with the kernels: train_data.parse, the oracle, and libzstd where the host has it.  No GPU and no emulator needed."""
import random

import pytest

import dict_build as db
import dict_edges as de
import dict_records as dr
import oracle
import train_data as td


@pytest.fixture(scope="module")
def dictionaries():
    return de.dictionaries()


def test_ncount_is_the_inverse_of_the_reader():
    """Random distributions at every accuracy log: zero runs of every length (the 2-bit repeat flags, 3 = go on), 'less than 1',
    and values on both sides of the short / long field boundary."""
    rng = random.Random(1)
    for log in (5, 6, 7, 8, 9):
        for _ in range(200):
            left, probs = 1 << log, []
            while left:
                kind = rng.random()
                if kind < 0.35 and len(probs) < 48:
                    probs += [0] * rng.choice((1, 2, 3, 4, 6, 7, 9))
                p = -1 if kind > 0.8 else rng.randint(1, max(1, min(left, rng.choice((1, 2, 5, left)))))
                probs.append(p)
                left -= 1 if p == -1 else p
            raw = db.ncount(probs, log)
            got, got_log, end = td._ncount(raw + b"\xAA" * 4, 0, 9)
            assert (got, got_log, end) == (probs, log, len(raw)), (probs, log)


def test_every_dictionary_parses_to_what_it_was_built_from(dictionaries):
    ids = set()
    for name, raw in dictionaries.items():
        spec, p = de.SPECS[raw], td.parse(raw)
        assert p["magic"] == db.MAGIC and p["id"] == spec["id"], name
        for f in ("of", "ml", "ll"):
            assert p[f] == (list(spec[f][0]), spec[f][1]), (name, f)
        assert p["rep"] == spec["rep"] and p["content"] == spec["content"], name
        if isinstance(spec["huf"], (bytes, bytearray)):
            w, end = td._huffman_weights(spec["huf"], 0)
            assert end == len(spec["huf"]) and p["weights"] == w, name
        else:
            assert p["weights"][:-1] == list(spec["huf"]) and p["weights"][-1] > 0, name
        assert spec["id"] not in ids, name
        ids.add(spec["id"])


def test_the_oracle_loads_every_dictionary(dictionaries):
    for name, raw in dictionaries.items():
        spec, od = de.SPECS[raw], oracle.Dictionary(raw)
        assert od.status == 0, (name, od.status)
        i = od.info
        assert i["id"] == spec["id"] and i["content_len"] == len(spec["content"]), name
        assert [i["hist0"], i["hist1"], i["hist2"]] == spec["rep"], name
        assert (i["of_log"], i["ml_log"], i["ll_log"]) == (spec["of"][1], spec["ml"][1], spec["ll"][1]), name


def test_libzstd_takes_every_dictionary_but_the_listed_ones(dictionaries):
    """libzstd decompresses a frame of its own making with each dictionary: one it compressed with that dictionary or, where its
    compressor asks more of a dictionary than its decoder does (dict_build.LIBZSTD_COMPRESSOR_REFUSES, an explicit list: huf_direct,
    whose Huffman code lacks symbols), one it compressed with the bare content as a raw-content dictionary (same matches into the content; repeat offsets 1, 4, 8).
    The dictionaries of dict_build.LIBZSTD_REFUSES (content sizes 0 and 3: a repeat offset larger than the content) its decoder must
    refuse."""
    assert set(db.LIBZSTD_REFUSES) <= set(dictionaries) and all(n.startswith("content_") for n in db.LIBZSTD_REFUSES)
    if not dr.libzstd():
        return
    z, cctx, _ = dr.libzstd()
    import ctypes
    for name, raw in dictionaries.items():
        spec = de.SPECS[raw]
        sample = b"a sample that libzstd compresses with the dictionary; " * 4 + spec["content"][-48:]
        cap = z.ZSTD_compressBound(len(sample))
        out = ctypes.create_string_buffer(cap)
        r = z.ZSTD_compress_usingDict(cctx, out, cap, sample, len(sample), raw, len(raw), 3)
        if name in db.LIBZSTD_REFUSES:
            assert z.ZSTD_isError(r), f"{name}: libzstd was expected to refuse it ({db.LIBZSTD_REFUSES[name]})"
            plain = dr.zstd_compress_dict(sample, b"", 3)
            assert dr.zstd_decompress_dict(plain, len(sample), None) == sample
            assert dr.zstd_decompress_dict(plain, len(sample), raw) is None, name
            continue
        assert bool(z.ZSTD_isError(r)) == (name in db.LIBZSTD_COMPRESSOR_REFUSES), name
        if name in db.LIBZSTD_COMPRESSOR_REFUSES:
            assert spec["rep"] == [1, 4, 8] and len(spec["content"]) >= 8, name
            frame = dr.zstd_compress_dict(sample, spec["content"], 3)
        else:
            frame = out.raw[:r]
        assert dr.zstd_decompress_dict(frame, len(sample), raw) == sample, name
