"""Edge inputs of the records level with dictionaries (CZ_COMPRESS_RECORDS, cz_compress_records_dict_kernel): hand-built
dictionaries (dict_build through dict_edges.full) and records of at most 32 KiB that each reach one branch of the dictionary path
under this level's parse — three candidates per position (the chunk, the wave's own 12-bit table, the dictionary's table), one
block per frame, no reference to the dictionary's repeat offsets.  Where an input of dict_edges reaches its branch under this parse
too it is taken from there with its predicate; the others are built here.  Each edge comes with a predicate on the analysed frame
(compress_edges.analyse with dictionary=), so an input that stops reaching its branch fails.  Test infrastructure only."""
import functools

import compress_edges as ce
import dict_edges as de
from dict_edges import Edge

RECORD_MAX = 32 << 10
# edges of dict_edges whose inputs and predicates hold under this level's parse as they stand
TAKEN = ("ends_at_boundary_4", "ends_at_boundary_8", "across_boundary_5", "across_boundary_8",
         "across_boundary_long_5_300", "across_boundary_long_32_300", "across_boundary_long_33_300",
         "content_window_exact", "content_window_plus1", "content_0", "content_3", "content_4", "content_8",
         "huf_direct_128", "huf_direct_128_miss", "huf_deep_1023", "huf_deep_1024", "id_0", "id_255", "id_256", "id_65535", "id_65536")


def _seq_is(i, ll, ml, ofv, off):
    def chk(fr):
        (b,) = fr["blocks"]
        assert b["type"] == "compressed" and len(b["seqs"]) > i, b["type"]
        assert b["seqs"][i] == (ll, ml, ofv) and b["offsets"][i] == off, (b["seqs"][i], b["offsets"][i])
    return chk


def candidate_edges():
    E, D = [], 200
    # a source that only the dictionary's table knows: 100 fresh bytes, then the content's last 16
    g = de._content_gen(2000, D, 16)
    c = g.bytes()
    de._tail(g.lit(100).copy(116, 16))
    E.append(Edge("dict_table_only", "cand_a", de.full(0x6001, c), g.bytes()[D:], _seq_is(0, 100, 16, 116 + 3, 116)))
    # the same 16 bytes at input position 0 and again at 116, in the next chunk: the wave's own table is asked before the
    # dictionary's and answers with the nearer source (offset 116; the content's copy lies 132 back)
    for seed in range(2010, 2400, 10):
        g = de._content_gen(seed, D, 16)
        c = g.bytes()
        g.copy(16, 16).lit(100).copy(116, 16)
        data = de._tail(g).bytes()[D:]
        h = de.hashes(data) >> 2
        if not any(int(x) == int(h[0]) for x in h[1:116]):              # position 0 is still the entry of its 12-bit bucket
            break
    E.append(Edge("own_table_wins", "cand_b", de.full(0x6002, c), data, _seq_is(1, 100, 16, 116 + 3, 116)))
    return E


def fse_edges():
    """A dictionary table without a state for a code the record needs: that field is Predefined, the other two stay Repeat."""
    E = []
    c = ce.Gen(40).lit(64, alphabet=range(0x80, 0x100)).bytes()         # a content nothing below matches
    for i, (name, kw, first, want) in enumerate((
            ("sparse_ll", {"ll": ([4] * 16, 6)}, [("lit", 20), ("copy", 8, 20)], (0, 3, 3)),                     # LL code 18
            ("sparse_of", {"of": ([3] * 10 + [2], 5)}, [("lit", 3000), ("copy", 2500, 20)], (3, 0, 3)),         # OF code 11
            ("sparse_ml", {"ml": ([2] * 32, 6)}, [("lit", 10), ("copy", 8, 50)], (3, 3, 0)))):                   # ML code 38
        d = de.full(0x6100 + i, c, **kw)
        for tag, steps, w in (("", first, want), ("_unneeded", [("lit", 10), ("copy", 8, 20)], (3, 3, 3))):
            g = ce.Gen(2500 + 2 * i + len(tag))
            for op, *a in steps:
                getattr(g, op)(*a)
            g.lit(10).copy(25, 20).lit(12).copy(30, 30).lit(9).copy(40, 24)
            de._skew(g, 400)                                            # compressible literals behind the last sequence

            def chk(fr, w=w):
                (b,) = fr["blocks"]
                assert b["type"] == "compressed" and de.modes(b) == w, (b["type"], de.modes(b))
            E.append(Edge(f"rec_{name}{tag}", f"rec_{name}", d, g.bytes(), chk))
    return E


def log_edges():
    """Accuracy logs 9 / 9 / 8 and 5 / 5 / 5: every field in Repeat_Mode with tables of the largest and the smallest size."""
    c = ce.Gen(40).lit(64, alphabet=range(0x80, 0x100)).bytes()
    dmax = de.full(0x6200, c, of=de.MAX_OF, ml=de.MAX_ML, ll=de.MAX_LL)
    dmin = de.full(0x6201, c, of=de.MIN_OF, ml=de.MIN_ML, ll=de.MIN_LL)

    def all_repeat(least):
        def chk(fr):
            (b,) = fr["blocks"]
            assert b["type"] == "compressed" and len(b["seqs"]) >= least and de.modes(b) == (3, 3, 3), (b["type"], de.modes(b))
        return chk
    # LL codes 0-31, ML codes 16-39, any offset: what the 5 / 5 / 5 tables hold
    g = ce.Gen(2600).lit(60).copy(50, 20).lit(12).copy(30, 30).lit(9).copy(40, 24).lit(40).copy(100, 60).lit(8)
    small = g.bytes()
    g = ce.Gen(2601)
    for k in range(70):                                                 # more than one round of 64 sequences
        g.lit(5 + k % 7).copy(4 + k % 3, 19 + k % 16)
    many = g.lit(8).bytes()
    return [Edge("rec_logs_max_small", "rec_logs_max", dmax, small, all_repeat(4)),
            Edge("rec_logs_max_many", "rec_logs_max", dmax, many, all_repeat(65)),
            Edge("rec_logs_max_ladder", "rec_logs_max", dmax, ce.corpus_text(RECORD_MAX), all_repeat(1000)),
            Edge("rec_logs_min_small", "rec_logs_min", dmin, small, all_repeat(4)),
            Edge("rec_logs_min_many", "rec_logs_min", dmin, many, all_repeat(65))]


def repeat_edges():
    """The first sequence of the block has the dictionary's first repeat offset and literals in front of it: the plain dictionary
    compressor writes Offset_Value 1, this level the offset itself."""
    D = 200
    g = de._content_gen(1300, D, 16)
    c = g.bytes()
    de._tail(g.lit(5).copy(21, 16))
    return [Edge("rec_rep0_explicit", "rec_rep_21", de.full(0x6301, c, rep=(21, 4, 8)), g.bytes()[D:], _seq_is(0, 5, 16, 21 + 3, 21))]


@functools.lru_cache(maxsize=None)
def edges():
    """[Edge], deterministic; every input at most 32 KiB."""
    by_name = {e.name: e for e in de.edges()}
    E = [by_name[n] for n in TAKEN] + candidate_edges() + fse_edges() + log_edges() + repeat_edges()
    assert len({e.name for e in E}) == len(E) and all(len(e.data) <= RECORD_MAX for e in E)
    return E


def manifest_batch():
    """(buffers, dict_index) of the sha256 manifest tests/golden/compress_records/manifest.json
    (scripts/gen_compress_records_manifest.py): dict_records.manifest_batch() restricted to inputs of at most 32 KiB."""
    import dict_records as dr
    bufs, idx = dr.manifest_batch()
    keep = [i for i, b in enumerate(bufs) if len(b) <= RECORD_MAX]
    return [bufs[i] for i in keep], [idx[i] for i in keep]
