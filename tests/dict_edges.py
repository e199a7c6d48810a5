"""Edge inputs of the dictionary compressor (cz_enc_dict_prep_kernel, cz_compress_frames_dict_kernel): hand-built dictionaries
(dict_build) and inputs that each reach one place where the dictionary path differs from the plain one — the content / input
boundary, the 1 MiB window against the content, a dictionary FSE table without a state for a code, the compact encode tables at
their limits, Treeless literals against a partial or deep Huffman code, tiny contents, the Dictionary_ID widths.  Each edge comes
with a predicate on the analysed frame (compress_edges.analyse with dictionary=), so an input that stops reaching its branch fails.
Everything is rebuilt deterministically here; only the sha256 of the frames is committed
(tests/golden/compress_dict_edges/manifest.json).  Test infrastructure only.

The prepared hash table keeps one content position per bucket, the highest; every content below is built so that the position its
edge is about is that survivor (survivor(), checked when the edge is built)."""
import functools
import random
from dataclasses import dataclass
from typing import Callable

import numpy as np

import compress_edges as ce
import compress_fse as fx
import dict_build as db
import dict_records as dr
import train_data as td

KIB, MIB, BLOCK, WINDOW = ce.KIB, ce.MIB, ce.BLOCK, ce.WINDOW

# tables with a state for every code: one symbol takes what the others leave
FULL_LL = ([29] + [1] * 35, 6)
FULL_ML = ([12] + [1] * 52, 6)
FULL_OF = ([4] + [1] * 28, 5)
# accuracy logs 9 / 9 / 8: one symbol with more than half of the states (a count that is no power of two), one with a single
# ordinary state, one with a power of two, one with three states, every other symbol "less than 1"
MAX_LL = ([412, 1, 64, 3] + [-1] * 32, 9)
MAX_ML = ([-1, 395, 1, 64, 3] + [-1] * 48, 9)
MAX_OF = ([-1, -1, 1, 64, 3, 163] + [-1] * 23, 8)
# accuracy logs 5 / 5 / 5: 32 states cannot hold the 36 LL or the 53 ML codes, so these tables have the codes their records use
# (fx.skewed_ml, fx.gapped_codes and fx.fixed_copies: LL 0-31, ML 16-39 behind a run of sixteen zeros, OF 0-20) and no others
MIN_LL = ([1] * 32, 5)
MIN_ML = ([0] * 16 + [2] * 8 + [-1] * 4 + [1] * 12, 5)
MIN_OF = ([2] * 11 + [1] * 6 + [-1] * 4, 5)

# direct-form Huffman code of symbols 0..128 (128 weights, the weight of symbol 128 implied: 8).  Code lengths 11 - weight:
# 5 bits for 0x60-0x6F, 7 bits for 0x40-0x5F, 9 bits for 0x10-0x3F, 10 bits for 0x00-0x0F and 0x70-0x7F, 3 bits for 0x80.
DIRECT_W = [1] * 16 + [2] * 48 + [4] * 32 + [6] * 16 + [1] * 16
HUF5 = range(0x60, 0x70)            # the 5-bit symbols
HUF10 = range(0x70, 0x80)           # 10-bit symbols


@dataclass
class Edge:
    name: str
    dname: str                  # the name of its dictionary (dict_build.LIBZSTD_REFUSES is keyed by it)
    dictionary: bytes
    data: bytes
    check: Callable             # check(analysed frame): asserts the branch the input is there to reach
    emu: bool = True            # False: too slow for the CPU emulator; the GPU test holds it to the oracle and its predicate only
    header: tuple = None        # (width of the Dictionary_ID field, its value) where the edge is about it


# ------------------------------------------------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def golden():
    """The Huffman description (an FSE-compressed one of 256 symbols, 11 bits deep) and the tables of the first family dictionary."""
    raw = dr.dictionaries()[0]
    d = td.parse(raw)
    _, end = td._huffman_weights(raw, 8)
    assert d["max_bits"] == 11 and raw[8] < 128
    return {"huf": raw[8:end], "of": d["of"], "ml": d["ml"], "ll": d["ll"], "weights": d["weights"]}


SPECS = {}                          # dictionary bytes -> the arguments dict_build.build was given


def build(dict_id, huf, of, ml, ll, rep, content):
    raw = db.build(dict_id, huf, of, ml, ll, rep, content)
    SPECS[raw] = {"id": dict_id, "huf": huf, "of": of, "ml": ml, "ll": ll, "rep": list(rep), "content": bytes(content)}
    return raw


def full(dict_id, content, rep=(1, 4, 8), huf=None, of=FULL_OF, ml=FULL_ML, ll=FULL_LL):
    return build(dict_id, golden()["huf"] if huf is None else huf, of, ml, ll, rep, content)


def hashes(b):
    """The encoder's hash of every 4-byte window of b."""
    a = np.frombuffer(bytes(b), dtype=np.uint8).astype(np.uint64)
    key = a[:-3] | (a[1:-2] << 8) | (a[2:-1] << 16) | (a[3:] << 24)
    return ((key * 2654435761) & 0xFFFFFFFF) >> 18


def prepared_table(content):
    """The hash table cz_enc_dict_prep_kernel must leave: entry h = 1 + the highest content position v with v + 4 <= D, D - v <= 1 MiB
    and hash h; 0 where there is none."""
    D = len(content)
    lo = max(0, D - WINDOW)
    tab = np.zeros(1 << 14, dtype=np.uint32)
    if D - lo >= 4:
        h = hashes(content[lo:])
        tab[h] = np.arange(lo + 1, lo + 1 + len(h), dtype=np.uint32)     # ascending: the highest position is written last
    return tab


def survivor(content, v):
    """Content position v is the entry of its bucket in the prepared table: inside the last 1 MiB and no later position of the
    content has its hash."""
    D = len(content)
    lo = max(0, D - WINDOW)
    if v < lo or v + 4 > D:
        return False
    h = hashes(content[lo:])
    return not np.any(h[v - lo + 1:] == h[v - lo])


def modes(blk):
    m = blk["seq"]["modes"]
    return None if m is None else (m >> 6, (m >> 4) & 3, (m >> 2) & 3)      # (LL, OF, ML); 0 Predefined, 3 Repeat


def _compressed(fr):
    return [b for b in fr["blocks"] if b["type"] == "compressed"]


def _first(fr):
    b = fr["blocks"][0]
    assert b["type"] == "compressed" and b["seqs"], b["type"]
    return b["seqs"][0], b["offsets"][0]


def _content_gen(seed, n, k):
    """A Gen holding n unique bytes whose position n - k survives (the content); go on from it to build the input behind it."""
    for s in range(seed, seed + 4000, 40):
        g = ce.Gen(s).lit(n)
        if survivor(g.bytes(), n - k):
            return g
    raise RuntimeError("no content")


def _tail(g):
    """Something that makes the block worth compressing: a 40-byte copy from 20 back, between fresh bytes."""
    return g.lit(30).copy(20, 40).lit(8)


# --------------------------------------------------------------------------------------------------------- content / input boundary
def _seq0_is(ll, ml, ofv, off):
    def chk(fr):
        s, o = _first(fr)
        assert s == (ll, ml, ofv) and o == off, (s, o)
    return chk


def boundary_edges():
    E, D = [], 200
    for k in (4, 5, 6, 7, 8, 12):                                       # a match that ends where the content ends
        g = _content_gen(1000 + k, D, k)
        c = g.bytes()
        _tail(g.copy(k, k))
        E.append(Edge(f"ends_at_boundary_{k}", f"bnd_{k}", full(0x1100 + k, c), g.bytes()[D:], _seq0_is(0, k, k + 3, k)))
    for k in (5, 6, 7, 8):                                              # ... that runs across it, below CZE_CAP
        g = _content_gen(1100 + k, D, k)
        c = g.bytes()
        _tail(g.copy(k, 24))
        E.append(Edge(f"across_boundary_{k}", f"bnd_a{k}", full(0x1200 + k, c), g.bytes()[D:], _seq0_is(0, 24, k + 3, k)))
    for k in (5, 8, 31, 32, 33):                                        # ... through the extension loop
        g = _content_gen(1200 + k, D, k)
        c = g.bytes()
        d = full(0x1300 + k, c)
        for n in (300, 70000):
            data = (c[D - k:] * (n // k + 1))[:n]

            def chk(fr, n=n, k=k):
                s, o = _first(fr)
                assert s == (0, n, k + 3) and o == k and len(fr["blocks"]) == 1, (s, o)
                assert (52 in fr["blocks"][0]["ml_codes"]) == (n >= 65539) and modes(fr["blocks"][0]) == (3, 3, 3)
            E.append(Edge(f"across_boundary_long_{k}_{n}", f"bnd_l{k}", d, data, chk))
    # repeat offsets of the dictionary that point into its content
    g = _content_gen(1300, D, 16)
    c = g.bytes()
    _tail(g.lit(5).copy(21, 16))
    E.append(Edge("rep0_into_content", "rep_21", full(0x1401, c, rep=(21, 4, 8)), g.bytes()[D:], _seq0_is(5, 16, 1, 21)))
    g = _content_gen(1310, D, 16)
    c = g.bytes()
    g.copy(16, 16).lit(10).copy(16, 12).lit(30).copy(20, 40).lit(8)

    def rep0_ll0(fr):
        (s0, s1), (o0, o1) = fr["blocks"][0]["seqs"][:2], fr["blocks"][0]["offsets"][:2]
        assert s0 == (0, 16, 16 + 3) and o0 == 16, s0                    # never Offset_Value 1..3 with no literals
        assert s1[0] > 0 and s1[2] == 1 and o1 == 16, s1                 # the same distance behind literals: the repeat
    E.append(Edge("rep0_ll0", "rep_16", full(0x1402, c, rep=(16, 4, 8)), g.bytes()[D:], rep0_ll0))
    # a Raw block (with a sequence the decoder never sees) leaves the dictionary's history alone
    for seed in range(1320, 1400):
        g = ce.Gen(seed).lit(2100)
        c = g.bytes()
        g.lit(5000).copy(8, 5).lit(BLOCK - 5005)
        g.lit(100).copy(2000, 16).lit(100).copy(2000, 16).lit(50)
        data = g.bytes()[2100:]
        h = hashes(data[:BLOCK + 700])
        at = BLOCK + 100 - 2000
        if not np.any(h[at + 1:BLOCK + 100] == h[at]):                   # the source of the first match stays in the table
            break

    def rep_after_raw(fr):
        a, b = fr["blocks"]
        assert a["type"] == "raw" and b["type"] == "compressed"
        assert b["seqs"][0][0] > 0 and b["seqs"][0][2] == 1 and b["offsets"][0] == 2000, b["seqs"][:2]
    E.append(Edge("rep_after_raw_dict", "rep_2000", full(0x1403, c, rep=(2000, 4, 8)), data, rep_after_raw))
    return E


# ------------------------------------------------------------------------------------------------------------------- the window
def _zeros_with_marks(n, marks, seed):
    """n zero bytes with a mark of random non-zero bytes at each (position, length) of marks, every mark's start a survivor."""
    rng = random.Random(seed)
    while True:
        b = bytearray(n)
        ms = []
        for at, ln in marks:
            m = bytes(rng.randint(1, 255) for _ in range(ln))
            b[at:at + ln] = m
            ms.append(m)
        b = bytes(b)
        lo = max(0, n - WINDOW)
        if all(survivor(b, at) for at, _ in marks if at >= lo):
            return b, ms


class _AvoidGen(ce.Gen):
    """Gen whose new windows stay out of some hash buckets."""

    def lit_avoid(self, n, buckets, alphabet=range(1, 256)):
        alphabet = list(alphabet)
        for _ in range(n):
            tail = bytes(self.b[-3:])
            while True:
                x = self.rng.choice(alphabet)
                w = tail + bytes([x])
                if w not in self.seen and ce.enc_hash(w) not in buckets:
                    break
            self._push(x)
        return self


def window_edges():
    E = []
    D = MIB + 4096
    for name, at in (("content_window_exact", D - MIB), ("content_window_plus1", D - MIB - 1)):
        if at == D - MIB:
            c, (m,) = _zeros_with_marks(D, [(at, 16)], 21)
        else:                                                           # the same mark one byte earlier: just outside the window
            c = c[1:] + b"\0"
        data = _tail(ce.Gen(22).raw(m).lit(4, alphabet=range(1, 256))).bytes()
        if at == D - MIB:
            def chk(fr):
                s, o = _first(fr)
                assert s == (0, 16, MIB + 3) and o == MIB and 20 in fr["blocks"][0]["of_codes"], (s, o)
        else:
            def chk(fr):
                offs = [o for b in _compressed(fr) for o in b["offsets"]]
                assert offs and max(offs) <= MIB, offs
                assert fr["blocks"][0]["seqs"][0][0] >= 4, "a sequence covers input[0:4], whose source lies 1 MiB + 1 back"
        E.append(Edge(name, name, full(0x2001 + (at != D - MIB), c), data, chk))
    # a frame longer than the window stops reaching the content
    c, (m,) = _zeros_with_marks(4096, [(0, 32)], 23)
    g = _AvoidGen(24).raw(m)
    g.lit_avoid(MIB + 8 * KIB, {ce.enc_hash(m[:4])})
    data = g.bytes() + m

    def leaves(fr):
        assert not fr["header"]["single"] and fr["header"]["window"] == WINDOW
        s, o = _first(fr)
        assert s == (0, 32, 4096 + 3) and o == 4096, (s, o)
        assert sum(len(b["seqs"]) for b in fr["blocks"]) == 1, "the second mark is out of every match's reach"
    # emu=False: 1 MiB of incompressible input is 38 s of each emulator run, a third of the whole set's time
    E.append(Edge("content_leaves_window", "leaves", full(0x2003, c), data, leaves, emu=False))
    # a 3 MiB content: only its last MiB is in the table
    D = 3 * MIB
    spots = [(100, 32), (D - MIB - 40, 32), (D - MIB + 50, 32), (D - 500000, 32), (D - 100, 32)]
    c, ms = _zeros_with_marks(D, spots, 25)
    d = full(0x2004, c)
    for (at, _), m in zip(spots[2:], ms[2:]):
        E.append(Edge(f"big_content_last_{D - at}", "big", d, _tail(ce.Gen(26).raw(m).lit(4, alphabet=range(1, 256))).bytes(),
                      _seq0_is(0, 32, D - at + 3, D - at)))

    def none_into_content(fr):
        pos = 0
        for b in fr["blocks"]:
            assert b["type"] == "compressed" and b["seqs"]
            for (ll, ml, _), o in zip(b["seqs"], b["offsets"]):
                pos += ll
                assert o <= pos, (o, pos)
                pos += ml
    for i in (0, 1):
        E.append(Edge(f"big_content_first_{i}", "big", d, _tail(ce.Gen(27).raw(ms[i]).lit(4, alphabet=range(1, 256))).bytes(),
                      none_into_content))
    return E


# ---------------------------------------------------------------------------------------------------------------- content sizes
def content_size_edges():
    E, G = [], golden()
    rec = dr.records(3, seed=31)[0][1] + dr.records(3, seed=31)[4][1]   # two records of the first family
    assert rec[:8] == b'{"id": 0'

    def tables_used(fr):
        bl = _compressed(fr)
        assert any(b["lit"]["type"] == "treeless" for b in bl) and any(modes(b) == (3, 3, 3) for b in bl)

    for D, rep in ((0, (1, 4, 8)), (3, (1, 4, 8)), (4, (1, 2, 4)), (8, (1, 4, 8))):
        def chk(fr, D=D):
            tables_used(fr)
            if D >= 4:
                s, o = _first(fr)
                assert s[0] == 0 and o == D and s[1] >= D, (s, o)
            else:
                pos = 0
                for b in fr["blocks"]:
                    for (ll, ml, _), o in zip(b["seqs"], b["offsets"]):
                        pos += ll
                        assert o <= pos, (o, pos)
                        pos += ml
        E.append(Edge(f"content_{D}", f"content_{D}", build(0x3000 + D, G["huf"], G["of"], G["ml"], G["ll"], rep, rec[:D]), rec, chk))
    return E


# -------------------------------------------------------------------------------------------------------------------- FSE tables
def _skew(g, n):
    """n compressible literals (64 symbols, falling weights)."""
    return g.lit(n, list(range(0x30, 0x70)), [1.0 / (1 + i) ** 0.8 for i in range(64)])


def _two_blocks(seed, first):
    """Block 1: `first` (a list of Gen steps), compressible literals to the block's end; block 2: short literal runs, matches of 20
    and 30 bytes at short distances."""
    g = ce.Gen(seed)
    for op, *a in first:
        getattr(g, op)(*a)
    _skew(g, BLOCK - len(g.b))
    g.lit(10).copy(50, 20).lit(12).copy(30, 30).lit(9).copy(40, 24).lit(8)
    return g.bytes()


def _modes_are(*want):
    def chk(fr):
        got = [modes(b) for b in fr["blocks"]]
        assert all(b["type"] == "compressed" for b in fr["blocks"]) and got == list(want), got
    return chk


def fse_edges():
    E = []
    c = ce.Gen(40).lit(64, alphabet=range(0x80, 0x100)).bytes()         # a content nothing below matches
    plain = [("lit", 10), ("copy", 8, 20)]                              # LL 10, ML 20, offset 8: codes every table has
    for name, kw, first, want in (
            ("sparse_ll", {"ll": ([4] * 16, 6)}, [("lit", 20), ("copy", 8, 20)], (0, 3, 3)),                     # LL code 18
            ("sparse_of", {"of": ([3] * 10 + [2], 5)}, [("lit", 3000), ("copy", 2500, 20)], (3, 0, 3)),         # OF code 11
            ("sparse_ml", {"ml": ([2] * 32, 6)}, [("lit", 10), ("copy", 8, 50)], (3, 3, 0))):                    # ML code 38
        d = full(0x4000 + len(E), c, **kw)
        E.append(Edge(name, name, d, _two_blocks(41 + len(E), first), _modes_are(want, want)))
        E.append(Edge(name + "_unneeded", name, d, _two_blocks(51 + len(E), plain), _modes_are((3, 3, 3), (3, 3, 3))))
    # accuracy logs at their limits
    dmax = full(0x4100, c, of=MAX_OF, ml=MAX_ML, ll=MAX_LL)
    dmin = full(0x4101, c, of=MIN_OF, ml=MIN_ML, ll=MIN_LL)

    def all_repeat(inner=None, count=None):
        def chk(fr):
            bl = [b for b in _compressed(fr) if b["seqs"]]
            assert bl and all(modes(b) == (3, 3, 3) for b in bl), [modes(b) for b in bl]
            if inner:
                inner(fr)
            if count:
                assert len(fr["blocks"]) == 1 and bl[0]["seq"]["count"] == count[0] and bl[0]["seq"]["header_len"] == count[1], bl[0]["seq"]
        return chk
    for e in ce.code_ladders():
        E.append(Edge(f"logs_max_{e.name}", "logs_max", dmax, e.data, all_repeat(e.check)))
    for name, data in (("gapped", fx.gapped_codes()), ("skewed_ml", fx.skewed_ml())):
        E.append(Edge(f"logs_max_{name}", "logs_max", dmax, data, all_repeat()))
        E.append(Edge(f"logs_min_{name}", "logs_min", dmin, data, all_repeat()))
    E.append(Edge("logs_min_fixed", "logs_min", dmin, fx.fixed_copies(), all_repeat()))
    g = ce.Gen(45).lit(40).copy(20, 8).lit(1).copy(30, 8).lit(2).copy(25, 8).lit(3).copy(35, 8).lit(8)   # LL codes 1, 2, 3

    def short_ll(fr):
        assert {1, 2, 3} <= fr["blocks"][0]["ll_codes"], fr["blocks"][0]["seqs"]
    E.append(Edge("logs_max_short_ll", "logs_max", dmax, g.bytes(), all_repeat(short_ll)))
    for n in (127, 128, 0x7F00):
        E.append(Edge(f"logs_max_seqs_{n:#x}", "logs_max", dmax, ce.debruijn_tokens(ce.SEQ_LEN[n]),
                      all_repeat(count=(n, 1 if n < 128 else (2 if n < 0x7F00 else 3)))))
    return E


# ----------------------------------------------------------------------------------------------------------------------- Huffman
def _lit_types(*want):
    def chk(fr):
        got = [b["lit"]["type"] if b["type"] == "compressed" else b["type"] for b in fr["blocks"]]
        assert len(got) >= len(want) and all(w is None or g == w for g, w in zip(got, want)), got
        assert "treeless" not in got[len(want):], got
    return chk


def huffman_edges():
    E = []
    c = ce.Gen(60).lit(64, alphabet=range(0xC0, 0x100)).bytes()
    d = full(0x5000, c, huf=DIRECT_W)
    E.append(Edge("huf_direct_128", "huf_direct", d, ce.Gen(61).lit(200, HUF5).copy(8, 40).lit(8, HUF5).bytes(), _lit_types("treeless")))
    g = ce.Gen(61).lit(200, HUF5)
    g.b[100] = 129

    def no_treeless(fr):
        assert fr["blocks"][0]["type"] == "compressed" and fr["blocks"][0]["lit"]["type"] in ("raw", "huffman"), fr["blocks"][0]["lit"]
    E.append(Edge("huf_direct_128_miss", "huf_direct", d, g.copy(8, 40).lit(8, HUF5).bytes(), no_treeless))
    # Raw literals, Treeless, a tree of its own, and never Treeless after it
    g = ce.Gen(62).lit(20, HUF10)
    g.copy(8, BLOCK - 20)
    g.lit(200, HUF5).copy(8, BLOCK - 200)
    g.lit(2000, list(range(0x60, 0x70)) + [0x90, 0x91], [4] * 16 + [1, 1]).copy(8, BLOCK - 2000)
    g.lit(200, HUF5).copy(8, BLOCK - 200)
    g.lit(150, HUF5).copy(8, 100).lit(8, HUF5)
    E.append(Edge("huf_raw_treeless_own", "huf_direct", d, g.bytes(), _lit_types("raw", "treeless", "huffman")))
    # the 11-bit code of the golden dictionary (an FSE-compressed description of 256 symbols): 1023 and 1024 literals
    w = golden()["weights"]
    alpha = [s for s in range(256) if 12 - w[s] <= 8]
    weights = [2.0 ** -(12 - w[s]) for s in alpha]
    d = full(0x5001, c, huf=golden()["huf"])
    for n in (1023, 1024):
        data = next(x for x in (ce.Gen(s).lit(n, alpha, weights).copy(8, 40).bytes() for s in range(63, 99)) if x[n - 1] != x[n - 9])

        def chk(fr, n=n):
            lit = fr["blocks"][0]["lit"]
            assert lit["type"] == "treeless" and lit["regen"] == n and lit["streams"] == (1 if n < 1024 else 4), lit
        E.append(Edge(f"huf_deep_{n}", "huf_deep", d, data, chk))
    return E


# ------------------------------------------------------------------------------------------------------------------------ header
def header_edges():
    E = []
    g = _content_gen(70, 100, 8)
    c = g.bytes()
    data = _tail(g.copy(8, 8)).bytes()[100:]
    for did, width in ((0, 0), (255, 1), (256, 2), (65535, 2), (65536, 4)):
        E.append(Edge(f"id_{did}", f"id_{did}", full(did, c), data, _seq0_is(0, 8, 8 + 3, 8), header=(width, did)))
    return E


def check_header(edge, frame):
    import dict_frames as dfr
    if edge.header is not None:
        assert dfr.header_id(frame) == edge.header, (edge.name, dfr.header_id(frame))


# ------------------------------------------------------------------------------------------------------------------ the edge list
@functools.lru_cache(maxsize=None)
def edges():
    """[Edge], deterministic."""
    E = boundary_edges() + window_edges() + content_size_edges() + fse_edges() + huffman_edges() + header_edges()
    assert len({e.name for e in E}) == len(E)
    assert sum(not e.emu for e in E) <= 2
    assert {e.dname for e in E if e.dname in db.LIBZSTD_REFUSES} == set(db.LIBZSTD_REFUSES)
    return E


def dictionaries(E=None):
    """{dictionary name: bytes} of the edges, in first-use order."""
    out = {}
    for e in (edges() if E is None else E):
        assert out.setdefault(e.dname, e.dictionary) == e.dictionary, e.dname
    return out


def batch(E):
    """(buffers, raw dictionaries, index per buffer) for the runners."""
    names = list(dictionaries(E))
    return [e.data for e in E], [dictionaries(E)[n] for n in names], [names.index(e.dname) for e in E]


def treeless_size(weights, hist_of_stream):
    """Bytes of one Huffman stream: the literals' code lengths (max_bits + 1 - weight), the closing bit, rounded up."""
    mb = sum(1 << (x - 1) for x in weights if x).bit_length() - 1
    bits = sum(n * (mb + 1 - weights[s]) for s, n in enumerate(hist_of_stream) if n)
    return bits // 8 + 1
