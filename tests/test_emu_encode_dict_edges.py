"""The dictionary compressor (cz_dict_setup_kernel -> cz_enc_dict_prep_kernel -> cz_compress_frames_dict_kernel, the unmodified
kernel sources) on the CPU SIMT emulator under ASan + UBSan, with the hand-built dictionaries and edge inputs of tests/dict_edges.py.
Every frame is held to two decoders that share no code with the kernel (the oracle and libzstd, each with the dictionary), to the
branch its input is there to reach, and every Treeless literal section to the size the dictionary's code lengths give.  No GPU
needed.

One edge is emu=False and runs on the GPU only: content_leaves_window, whose 1 MiB of incompressible input takes a third of an
emulator run of the whole set.  The 3 MiB content of big_content stays: preparing it takes under a second on the emulator, where
test_emu_encode_dict.test_cross_block_table_state emulates a 3 MiB input."""
import hashlib
import json
import os

import pytest

import compress_edges as ce
import dict_build as db
import dict_edges as de
import dict_records as dr
import emu_encode_dict_runner as emu
import oracle

pytestmark = pytest.mark.xdist_group(name="emu_encode_dict_edges")

FLAGS = (0, emu.CHECKSUM)
MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compress_dict_edges", "manifest.json")


@pytest.fixture(scope="module")
def edges():
    return [e for e in de.edges() if e.emu]


@pytest.fixture(scope="module")
def runs(edges):
    """{flags: [(edge, result record, whole output region, analysed frame)]}: one emulator run per flag set, shared.  A frame the
    oracle cannot read is kept with None for its analysis: test_frames_decode reports it, test_branch_predicates fails on it.
    "tables": the prepared hash table of every dictionary, in the order of de.dictionaries(edges); "why": analyse's message for
    each frame it could not read."""
    bufs, dicts, idx = de.batch(edges)
    out, why = {}, {}
    for flags in FLAGS:
        got, tables = emu.run(bufs, dicts, index=idx, flags=flags, tables=True)
        out.setdefault("tables", tables)
        rows = []
        for e, (r, region) in zip(edges, got):
            assert int(r["status"]) == 0, e.name
            try:
                fr = ce.analyse(region[:int(r["bytes_written"])], e.data, dictionary=e.dictionary)
            except AssertionError as ex:
                fr, why[(flags, e.name)] = None, f"analyse: {ex}"
            rows.append((e, r, region, fr))
        out[flags] = rows
    out["why"] = why
    return out


def _each(runs):
    for flags in FLAGS:
        for e, r, region, fr in runs[flags]:
            yield flags, e, r, region, fr


def test_prepared_tables(edges, runs):
    """cz_enc_dict_prep_kernel: one entry per bucket, the highest position of the content's last 1 MiB (contents of 0 to 3 MiB)."""
    import numpy as np
    import train_data as td
    for (name, raw), got in zip(de.dictionaries(edges).items(), runs["tables"]):
        want = de.prepared_table(td.parse(raw)["content"])
        assert np.array_equal(got, want), (name, int((got != want).sum()))


def test_frames_decode(runs):
    for flags, e, r, region, fr in _each(runs):
        n, b = int(r["bytes_written"]), e.data
        frame = region[:n]
        assert n <= emu.compress_bound(len(b)), (e.name, n)
        assert set(region[n:]) <= {0xEE}, f"{e.name}: bytes past bytes_written were touched"
        assert int(r["bytes_read"]) == len(b)
        st, out = oracle.decode_frame_with_dict(frame, oracle.Dictionary(e.dictionary), cap=len(b) + 64)
        assert st == 0 and out == b, (e.name, flags, st)
        assert fr is not None, (e.name, flags, runs["why"].get((flags, e.name)))
        assert fr["header"]["content_size"] == len(b) and fr["end"] == n, e.name
        assert fr["header"]["checksum"] == bool(flags & emu.CHECKSUM)
        if flags & emu.CHECKSUM:
            assert int.from_bytes(frame[-4:], "little") == oracle.xxh64(b) & 0xFFFFFFFF == int(r["checksum"]), e.name
        if dr.libzstd():
            got = dr.zstd_decompress_dict(frame, len(b), e.dictionary)
            if e.dname in db.LIBZSTD_REFUSES:
                assert got is None, f"{e.name}: libzstd was expected to refuse the dictionary"
            else:
                assert got == b, f"{e.name}: libzstd"


def test_branch_predicates(runs):
    for flags, e, r, region, fr in _each(runs):
        assert fr is not None, f"{e.name} (flags {flags}): the frame cannot be analysed: {runs['why'].get((flags, e.name))}"
        try:
            e.check(fr)
            de.check_header(e, region[:int(r["bytes_written"])])
        except AssertionError as ex:
            raise AssertionError(f"{e.name} (flags {flags}) misses its branch: {ex}") from ex


def test_window_and_offsets(runs):
    """No offset above 1 MiB (that it stays inside content + position, analyse asserts); Offset_Value 1 only behind literals."""
    for _, e, _, _, fr in _each(runs):
        for b in fr["blocks"] if fr else ():
            if b["type"] == "compressed":
                assert all(o <= ce.WINDOW for o in b["offsets"]), e.name
                assert all(ofv > 3 or (ofv == 1 and ll > 0) for ll, _, ofv in b["seqs"]), e.name


def test_treeless_sections_have_the_size_the_dictionarys_code_gives(runs):
    """Every Treeless section: its size recomputed from the dictionary's code lengths and the literals of each stream equals the
    size in its header, and it is smaller than the Raw section of the same literals."""
    import train_data as td
    weights, seen, streams = {}, set(), set()
    for _, e, _, _, fr in _each(runs):
        for i, b in enumerate(fr["blocks"] if fr else ()):
            if b["type"] != "compressed" or b["lit"]["type"] != "treeless":
                continue
            if e.dname not in weights:
                weights[e.dname] = td.parse(e.dictionary)["weights"]
            w, lits, lit = weights[e.dname], b["literals"], b["lit"]
            n = len(lits)
            assert n == lit["regen"] and lit["streams"] == (4 if n >= 1024 else 1), (e.name, i)
            seg = (n + 3) // 4 if n >= 1024 else n
            parts = [lits[k:k + seg] for k in range(0, n, seg)]
            assert len(parts) == lit["streams"]
            assert all(x < len(w) and w[x] for x in lits), (e.name, i)
            size = (6 if n >= 1024 else 0) + sum(de.treeless_size(w, [p.count(bytes([s])) for s in range(256)]) for p in parts)
            assert size == lit["comp"], (e.name, i, size, lit["comp"])
            assert lit["header_len"] + size < n + (1 if n < 32 else (2 if n < 4096 else 3)), (e.name, i)
            seen.add(e.name)
            streams.add(lit["streams"])
    assert seen >= {"content_0", "content_3", "content_4", "content_8", "huf_direct_128", "huf_raw_treeless_own", "huf_deep_1023",
                    "huf_deep_1024"} and streams == {1, 4}, sorted(seen)


def test_codes_cover_the_tables_at_accuracy_logs_9_9_8(runs):
    """Across the records of the logs_max dictionary, all written with its tables: every LL code 0-35 and every ML code 1-52 (code 0
    is a match of 3, shorter than the encoder's shortest)."""
    for flags in FLAGS:
        ll, ml = set(), set()
        for e, _, _, fr in runs[flags]:
            if e.dname == "logs_max" and fr:
                for b in fr["blocks"]:
                    if b["type"] == "compressed" and b["seqs"]:
                        assert de.modes(b) == (3, 3, 3), e.name
                        ll |= b["ll_codes"]
                        ml |= b["ml_codes"]
        assert ll == set(range(36)), sorted(set(range(36)) ^ ll)
        assert ml == set(range(1, 53)), sorted(set(range(1, 53)) ^ ml)


def test_reversed_batch_gives_the_same_frames(edges, runs):
    bufs, dicts, idx = de.batch(edges)
    got = emu.run(bufs[::-1], dicts[::-1], index=[len(dicts) - 1 - i for i in idx[::-1]])
    for (e, r, region, _), (r2, region2) in zip(runs[0], got[::-1]):
        assert int(r2["status"]) == 0 and int(r2["bytes_written"]) == int(r["bytes_written"]) and region2 == region, e.name


def test_frames_equal_the_manifest(edges, runs):
    m = json.load(open(MANIFEST))
    assert m["names"] == [e.name for e in edges]
    for flags in FLAGS:
        got = [hashlib.sha256(region[:int(r["bytes_written"])]).hexdigest() for _, r, region, _ in runs[flags]]
        bad = [e.name for e, g, w in zip(edges, got, m["flags"][str(flags)]) if g != w]
        assert not bad, (flags, bad)
