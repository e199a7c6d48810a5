"""Inputs and expectations for CZ_COMPRESS_HIGH.  Shares no code with the kernel: the inputs are built with
compress_edges.Gen, each construction is checked here in pure Python against a restatement of the default finder (the nearest
position with the same 4-byte hash among the 64 before it in the 256-byte chunk, else the one entry of the 2^14 table as it stood
before the chunk), and the expectations read the frames through compress_edges.analyse, which gives (LL, ML, Offset_Value) per
sequence through the oracle.  Test infrastructure only."""
import compress_edges as ce

BLOCK = ce.BLOCK
CHUNK, BACK = 256, 64
D1, D2 = 700, 1900


# ------------------------------------------------------------------------------------------------- the default finder, restated
def hash8(b8):
    """The second table's hash of an 8-byte key (zstd's 8-byte prime, 14 bits)."""
    return ((int.from_bytes(b8, "little") * 0xCF1BBCDCB7A56463) & 0xFFFFFFFFFFFFFFFF) >> 50


def finder(data):
    """position -> the candidate the default finder looks at there (one block; positions without a candidate are absent)."""
    assert len(data) <= BLOCK
    table, cand = {}, {}
    for c0 in range(0, len(data), CHUNK):
        hs = [ce.enc_hash(data[p:p + 4]) if p + 4 <= len(data) else None for p in range(c0, min(c0 + CHUNK, len(data)))]
        for t, h in enumerate(hs):
            if h is None:
                continue
            near = next((j for j in range(t - 1, max(t - BACK, 0) - 1, -1) if hs[j] == h), None)
            if near is not None and data[c0 + near:c0 + near + 4] == data[c0 + t:c0 + t + 4]:
                cand[c0 + t] = c0 + near
            elif near is None and h in table:
                cand[c0 + t] = table[h]
        for t, h in enumerate(hs):
            if h is not None:
                table[h] = c0 + t
    return cand


def match_len(data, p, src):
    n = 0
    while p + n < len(data) and data[p + n] == data[src + n]:
        n += 1
    return n


def nearest(data, p, n=4):
    """The nearest earlier position where the n bytes at p occur (overlapping p allowed), or -1."""
    return data.rfind(data[p:p + n], 0, p + n - 1)


def check_copies(data, copies, found=True):
    """Every (start, distance, length) is a copy that stands alone: its first four bytes occur nowhere nearer, it cannot start a byte
    earlier or run a byte longer, and (found) the default finder looks at exactly that source at its start."""
    cand = finder(data) if found else None
    for p, d, n in copies:
        assert data[p:p + n] == data[p - d:p - d + n], (p, d, n)
        assert nearest(data, p) == p - d, (p, d, nearest(data, p))
        assert data[p - 1] != data[p - 1 - d], (p, d, "starts earlier")
        assert match_len(data, p, p - d) == n, (p, d, n, match_len(data, p, p - d))
        if found:
            assert cand.get(p) == p - d, (p, d, cand.get(p))


class Built:
    """An input, the copies it was built from [(start, distance, length)] and the sites an expectation refers to."""

    def __init__(self, data, copies, sites=()):
        self.data, self.copies, self.sites = data, list(copies), list(sites)


def _seeded(build, first_seed):
    """The first seed from first_seed on whose construction passes its own check (deterministic)."""
    for seed in range(first_seed, first_seed + 400):
        try:
            return build(seed)
        except AssertionError:
            continue
    raise RuntimeError("no seed gives an unambiguous construction")


def _stands_alone(data, p, d, n):
    """check_copies for one copy, from the bytes around it: the table's one entry for its first four bytes is still its source's
    when its chunk begins, and no position of the chunk in front of it shares their hash."""
    c0 = p & ~(CHUNK - 1)
    h = ce.enc_hash(data[p:p + 4])
    return (p - d < c0 and data[p - 1] != data[p - 1 - d] and match_len(data, p, p - d) == n and nearest(data, p) == p - d
            and not any(ce.enc_hash(data[q:q + 4]) == h for q in range(p - d + 1, c0))
            and not any(ce.enc_hash(data[q:q + 4]) == h for q in range(max(c0, p - BACK), p)))


def _rounds(g, rounds, body):
    """`rounds` times body(g, k, copies, extra), which appends one round and lists its copies; a round with a copy that does not
    stand alone is taken back and built again with `extra` more random bytes in front.  Returns every copy."""
    copies = []
    for k in range(rounds):
        for extra in range(65):
            assert extra < 64, "no unambiguous round"
            start, state, mine = len(g.b), g.rng.getstate(), []
            body(g, k, mine, extra)
            data = g.bytes()
            if all(_stands_alone(data, *c) for c in mine):
                break
            for i in range(max(start - 3, 0), len(g.b) - 3):
                g.seen.discard(bytes(g.b[i:i + 4]))
            del g.b[start:]
            g.rng.setstate(state)
            g.rng.random()
        copies += mine
    return copies


def _copy(g, copies, d, n):
    copies.append((len(g.b), d, n))
    g.copy(d, n)


# ------------------------------------------------------------------------------------------------------------- repeat offsets
def two_offsets(rounds=200):
    """Rounds of 16 random bytes, 32 from D1 back, 16 random bytes, 32 from D2 back: after the first round every sequence repeats
    the offset before the last."""
    def body(g, k, copies, extra):
        g.lit(extra)
        _copy(g, copies, D1, 32)
        g.lit(16)
        _copy(g, copies, D2, 32)
        g.lit(16)
    g = ce.Gen(1000).lit(2048)
    copies = _rounds(g, rounds, body)
    data = g.bytes()
    check_copies(data, copies)
    return Built(data, copies)


def expect_two_offsets(fr, built):
    (blk,) = fr["blocks"]
    seqs = blk["seqs"]
    assert blk["type"] == "compressed" and len(seqs) >= len(built.copies)
    assert sum(1 for _, _, ofv in seqs if ofv == 2) >= 0.9 * len(seqs), [s for s in seqs if s[2] != 2][:8]
    assert not [s for s in seqs[2:] if s[2] - 3 in (D1, D2)], "an offset of the history was written in full"


def back_to_back(rounds=150):
    """Rounds of 16 random bytes, 32 from D1 back and at once 32 from D2 back."""
    def body(g, k, copies, extra):
        g.lit(extra)
        _copy(g, copies, D1, 32)
        _copy(g, copies, D2, 32)
        g.lit(16)
    g = ce.Gen(2000).lit(2048)
    copies = _rounds(g, rounds, body)
    data = g.bytes()
    check_copies(data, copies)
    return Built(data, copies)


def expect_back_to_back(fr, built):
    (blk,) = fr["blocks"]
    seqs = blk["seqs"]
    assert blk["type"] == "compressed" and len(seqs) == len(built.copies), (len(seqs), len(built.copies))
    for k in range(2, len(seqs), 2):                                    # from the second round on
        (ll_a, ml_a, ofv_a), (ll_b, ml_b, ofv_b) = seqs[k], seqs[k + 1]
        assert ll_a > 0 and ofv_a == 2 and ml_a == 32, (k, seqs[k])
        assert ll_b == 0 and ofv_b == 1 and ml_b == 32, (k, seqs[k + 1])


def minus_one(rounds=24):
    """Rounds of 16 random bytes, 32 from d back and at once 32 from d - 1 back, with a d of the round's own: the second sequence
    has no literals and its offset is history[0] - 1."""
    def body(g, k, copies, extra):
        g.lit(extra)
        _copy(g, copies, 300 + 11 * k, 32)
        _copy(g, copies, 300 + 11 * k - 1, 32)
        g.lit(16)
    g = ce.Gen(3000).lit(1024)
    copies = _rounds(g, rounds, body)
    data = g.bytes()
    check_copies(data, copies)
    return Built(data, copies)


def expect_minus_one(fr, built):
    (blk,) = fr["blocks"]
    seqs, offs = blk["seqs"], blk["offsets"]
    assert len(seqs) == len(built.copies)
    for k in range(0, len(seqs), 2):
        assert seqs[k][0] > 0 and seqs[k][2] > 3, (k, seqs[k])
        assert seqs[k + 1][0] == 0 and seqs[k + 1][2] == 3 and offs[k + 1] == offs[k] - 1, (k, seqs[k + 1])


def minus_one_at_1(rounds=24):
    """The sibling: a run of one byte (offset 1) and at once 32 bytes from d back.  history[0] is 1 where the second sequence
    starts, so Offset_Value 3 (history[0] - 1 = 0) must not be written.  Bytes below 64 occur in the runs only.  sites: where the
    copies start."""
    high = range(64, 256)

    def body(g, k, copies, extra):
        g.lit(extra, alphabet=high)
        g.raw(bytes([k]) * 40)
        d = 300 + 11 * k
        while min(g.b[len(g.b) - d:len(g.b) - d + 32]) < 64:              # a source without a run in it
            d += 1
        _copy(g, copies, d, 32)
        g.lit(16, alphabet=high)
    g = ce.Gen(4000).lit(1024, alphabet=high)
    copies = _rounds(g, rounds, body)
    data = g.bytes()
    check_copies(data, copies)
    for p, _, _ in copies:
        assert data[p - 40:p] == bytes([data[p - 1]]) * 40 and data[p - 41] != data[p - 1]
    return Built(data, copies, [p for p, _, _ in copies])


def expect_minus_one_at_1(fr, built):
    (blk,) = fr["blocks"]
    seqs, offs = blk["seqs"], blk["offsets"]
    assert not [s for s in seqs if s[0] == 0 and s[2] == 3], "Offset_Value 3 without literals while history[0] is 1"
    after_run = [k + 1 for k in range(len(seqs) - 1) if offs[k] == 1 and seqs[k][1] == 39]
    assert len(after_run) == len(built.sites)
    for k in after_run:
        assert seqs[k][0] == 0 and seqs[k][2] != 3, (k, seqs[k])


# ------------------------------------------------------------------------------------------------------------------ lazy parse
def lazy_sites(k=100):
    """k sites: position p has a 4-byte match (the token wxyz of source A, which goes on with other bytes) and p + 1 starts a
    60-byte match (source B: xyz and 57 known bytes behind a byte other than w).  Both sources lie more than a chunk in front of
    the site, nothing else takes their table entries, and p + 1 is inside p's chunk.  sites: [(p, position of A, position of B's x)]."""
    g, sites = ce.Gen(77), []
    g.lit(64)
    tries = 0
    while len(sites) < k:
        tries += 1
        assert tries < 20 * k, "no unambiguous site"
        start, state = len(g.b), g.rng.getstate()
        g.lit(4)
        a = len(g.b) - 4
        tok = bytes(g.b[a:a + 4])
        g.lit(12)
        g.lit(1, alphabet=[x for x in range(256) if x != tok[0]])
        b = len(g.b)
        g.raw(tok[1:]).lit(57)
        src = bytes(g.b[b:b + 60])
        g.lit(300 + g.rng.randrange(40))
        p = len(g.b)
        g.raw(tok[:1] + src).lit(16)
        data = g.bytes()
        c0 = p & ~(CHUNK - 1)
        ok = (p & (CHUNK - 1)) < CHUNK - 2 and b + 60 < c0
        for key_at, source in ((p, a), (p + 1, b)):                     # the one table entry is the source's
            h = ce.enc_hash(data[key_at:key_at + 4])
            ok = ok and not any(ce.enc_hash(data[q:q + 4]) == h for q in range(source + 1, c0))
            ok = ok and not any(ce.enc_hash(data[q:q + 4]) == h for q in range(max(c0, key_at - BACK), key_at))
        ok = ok and all(nearest(data, q) < 0 for q in range(p - 16, p))     # nothing to take in front of the site
        ok = ok and match_len(data, p, a) == 4 and match_len(data, p + 1, b) == 60 and data[p] != data[b - 1]
        if ok:
            sites.append((p, a, b))
        else:                                                           # take the attempt back
            for i in range(start, len(g.b) - 3):
                g.seen.discard(bytes(g.b[i:i + 4]))
            del g.b[start:]
            g.rng.setstate(state)
            g.rng.random()
    data = g.bytes()
    cand = finder(data)
    for p, a, b in sites:
        assert nearest(data, p) == a and nearest(data, p + 1) == b and cand.get(p) == a and cand.get(p + 1) == b, (p, a, b)
    return Built(data, [], sites)


def expect_lazy_sites(fr, built, high=True):
    """high: a sequence of at least 60 bytes starts at p + 1 of every site, behind at least one literal, and none of 4 bytes at p.
    not high (the CZ_COMPRESS_FSE_TABLES frame of the same input): a short sequence starts at p."""
    (blk,) = fr["blocks"]
    at, pos = {}, 0
    for ll, ml, _ in blk["seqs"]:
        pos += ll
        at[pos] = (ll, ml)
        pos += ml
    for p, _, _ in built.sites:
        if high:
            assert p not in at and p + 1 in at and at[p + 1][1] >= 60 and at[p + 1][0] >= 1, (p, at.get(p), at.get(p + 1))
        else:
            assert p in at and at[p][1] < 60 and p + 1 not in at, (p, at.get(p))
    if high:
        assert sum(1 for ll, ml in at.values() if ml >= 60 and ll >= 1) >= len(built.sites)


# ---------------------------------------------------------------------------------------------------------------- second table
def long_match_lost():
    """One place: 200 bytes that stand far back (F) start with four bytes that stand again, nearer, in front of other bytes (S).
    The 4-byte table's one entry is S's; the second table still has F.  sites: [(p, position of F, position of S)]."""
    def build(seed):
        g = ce.Gen(seed).lit(300)
        f = len(g.b)
        g.lit(200)
        far = bytes(g.b[f:f + 200])
        g.lit(600)
        s = len(g.b)
        g.raw(far[:4]).lit(20).lit(600)
        p = len(g.b)
        g.raw(far).lit(16)
        data = g.bytes()
        c0 = p & ~(CHUNK - 1)
        assert nearest(data, p) == s and finder(data).get(p) == s and match_len(data, p, s) < 8 and match_len(data, p, f) == 200
        h = hash8(data[p:p + 8])
        assert not any(hash8(data[q:q + 8]) == h for q in range(f + 1, c0)), "the second table's entry is taken"
        return Built(data, [(p, p - f, 200)], [(p, f, s)])
    return _seeded(build, 5000)


def expect_long_match_lost(fr, built):
    ((p, f, _),) = built.sites
    (blk,) = fr["blocks"]
    pos = 0
    for (ll, ml, _), off in zip(blk["seqs"], blk["offsets"]):
        pos += ll
        if pos == p:
            assert ml >= 200 and off == p - f, (ll, ml, off)
            return
        pos += ml
    raise AssertionError("no sequence starts at the place")


# ------------------------------------------------------------------------------------------------------------- several blocks
TWO_BLOCKS_LEN = 140000
FAR = 5000                      # the table still holds most of what lies this far back


def two_blocks():
    """140 000 bytes.  Block 1 ends on offset 2000; block 2 starts with literals and a copy from 2000 back (the repeat offset is
    carried across the boundary, and the source lies in block 1), then has a copy from FAR back, out of block 1 too."""
    g = ce.mixed(BLOCK, 31, gen=True)
    g.lit(500)
    rep_at = len(g.b)
    g.copy(2000, 64).lit(300)
    far_at = len(g.b)
    g.copy(FAR, 64)
    while len(g.b) < TWO_BLOCKS_LEN:
        g.lit(min(2000, TWO_BLOCKS_LEN - len(g.b)))
        if len(g.b) + 64 <= TWO_BLOCKS_LEN:
            g.copy(2000, 64)
    data = g.bytes()
    assert len(data) == TWO_BLOCKS_LEN
    return Built(data, [(rep_at, 2000, 64), (far_at, FAR, 64)], [rep_at, far_at])


def expect_two_blocks(fr, built):
    a, b = fr["blocks"]
    rep_at, far_at = built.sites
    assert a["type"] == b["type"] == "compressed" and a["offsets"][-1] == 2000
    ll, ml, ofv = b["seqs"][0]
    assert ll == rep_at - BLOCK and ofv == 1 and ml >= 64 and b["offsets"][0] == 2000      # carried across the boundary
    pos, reach = BLOCK, []
    for (ll, ml, _), off in zip(b["seqs"], b["offsets"]):
        pos += ll
        if pos - off < BLOCK:
            reach.append((pos, off))
        pos += ml
    assert (rep_at, 2000) in reach and [1 for p, off in reach if off == FAR and far_at <= p < far_at + 32], reach[:4]


def raw_then_compressed():
    """A first block that comes out Raw although it has a sequence (5 bytes at offset 12), then a block whose first sequences use
    offset 12: compress_edges' rep_after_raw at this level, with an offset the start history (1, 4, 8) does not hold.  A Raw first
    block is a whole block, so this input cannot be smaller than 128 KiB."""
    g = ce.Gen(41).lit(5000).copy(12, 5).lit(BLOCK - 5005)
    g.lit(100).copy(12, 16).lit(100).copy(12, 16).lit(50)
    return Built(g.bytes(), [])


def expect_raw_then_compressed(fr, built):
    a, b = fr["blocks"]
    assert a["type"] == "raw" and b["type"] == "compressed"
    (ll0, _, ofv0), (ll1, _, ofv1) = b["seqs"][:2]
    assert ll0 > 0 and ofv0 == 12 + 3, b["seqs"][:2]                     # not a repeat offset: the Raw block left no history
    assert ll1 > 0 and ofv1 == 1, b["seqs"][:2]


def constructed():
    """name -> (Built, expectation) of every constructed input of one block."""
    return {
        "two_offsets": (two_offsets(), expect_two_offsets),
        "back_to_back": (back_to_back(), expect_back_to_back),
        "minus_one": (minus_one(), expect_minus_one),
        "minus_one_at_1": (minus_one_at_1(), expect_minus_one_at_1),
        "lazy_sites": (lazy_sites(), expect_lazy_sites),
        "long_match_lost": (long_match_lost(), expect_long_match_lost),
    }
