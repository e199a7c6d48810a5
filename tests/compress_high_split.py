"""Inputs and expectations for CZ_COMPRESS_HIGH_SPLIT.  Shares no code with the kernel: a model of the offset history
a segment may rely on, a check of how far back a later segment's matches reach, and two constructed inputs built with
compress_edges.Gen the way tests/compress_high.py builds its own.  The frames are read through compress_edges.analyse, which gives
(LL, ML, Offset_Value) per sequence and the offset the decoder resolves it to, through the oracle.  Test infrastructure only."""
import compress_edges as ce
import compress_high as ch

BLOCK = ce.BLOCK
D1, D2 = ch.D1, ch.D2
WINDOW = 1 << 20


def segments_of(an, S):
    """The blocks of an analysed frame, one list per segment of S input bytes."""
    segs = []
    for blk in an["blocks"]:
        k = blk["start"] // S
        while len(segs) <= k:
            segs.append([])
        segs[k].append(blk)
    return segs


# ------------------------------------------------------------------------------------------- the history a segment may rely on
def check_history(an, S):
    """Walks the (ll, ml, Offset_Value) triples of every segment with the history the segment itself can know: (1, 4, 8) for segment
    0, (0, 0, 0) — nothing known — for a later one, updated by the six cases of RFC 8878 §3.1.1.5.  (a) every Offset_Value <= 3
    resolves to an entry the model knows; (b) an Offset_Value > 3 never names an offset the model holds in a place usable at that
    literal length; and what the model resolves is what the decoder resolves, so the known entries are a prefix of the real history.
    Returns, per segment, how often each Offset_Value 1..3 occurs."""
    counts = []
    for k, blocks in enumerate(segments_of(an, S)):
        h = [1, 4, 8] if k == 0 else [0, 0, 0]
        used = {1: 0, 2: 0, 3: 0}
        for blk in blocks:
            for i, ((ll, ml, ofv), real) in enumerate(zip(blk["seqs"], blk.get("offsets", []))):
                where = (k, blk["start"], i, (ll, ml, ofv), tuple(h))
                usable = [h[0], h[1], h[2]] if ll else [h[1], h[2], h[0] - 1 if h[0] else 0]
                if ofv <= 3:
                    off = usable[ofv - 1]
                    assert off > 0, ("a repeat code on an entry the segment cannot know", where)
                    used[ofv] += 1
                    r = ofv - (1 if ll else 0)                          # 0 rep1, 1 rep2, 2 rep3, 3 rep1 - 1
                    if r == 1:
                        h = [h[1], h[0], h[2]]
                    elif r >= 2:
                        h = [off, h[0], h[1]]
                else:
                    off = ofv - 3
                    assert off not in [u for u in usable if u > 0], ("an offset of the known history was written in full", where)
                    h = [off, h[0], h[1]]
                assert off == real, ("the model and the decoder disagree", where, real)
        counts.append(used)
    return counts


def check_reach(an, S, W):
    """No match of a later segment starts in front of the overlap: p - offset >= max(0, s0 - W); and every offset stays within the
    1 MiB window."""
    for k, blocks in enumerate(segments_of(an, S)):
        lo = max(0, k * S - W) if k else 0
        for blk in blocks:
            pos = blk["start"]
            for (ll, ml, _), off in zip(blk["seqs"], blk.get("offsets", [])):
                pos += ll
                assert off <= WINDOW and pos - off >= lo, (k, pos, off, lo)
                pos += ml


def first_sequences(an, S):
    """Per segment the first sequence (ll, ml, Offset_Value) of its first Compressed block with sequences, or None."""
    out = []
    for blocks in segments_of(an, S):
        out.append(next((blk["seqs"][0] for blk in blocks if blk["seqs"]), None))
    return out


# ---------------------------------------------------------------------------------------------------------- constructed inputs
def two_offsets_across_cuts(S, tail=20000):
    """compress_high.two_offsets over three segments: rounds of 32 bytes from D1 back, 16 random bytes, 32 from D2 back, 16 random
    bytes.  In front of each cut random bytes fill up so that a round starts exactly at the cut, and the third byte of its first copy
    is broken: the first sequence behind the cut has literals and continues the copy from D1 back, which the unsplit frame writes as
    a repeat code.  sites: the cuts."""
    g = ce.Gen(1000).lit(2048)
    cuts = [S, 2 * S]
    total = 2 * S + tail
    while len(g.b) < total:
        cut = next((c for c in cuts if len(g.b) <= c < len(g.b) + 96), None)
        if cut is not None:
            g.lit(cut - len(g.b))
            g.copy(D1, 3)
            g.b[cut + 2] ^= 0x55                                        # later copies take the broken byte along
            g.copy(D1, 29)
        else:
            g.copy(D1, 32)
        g.lit(16).copy(D2, 32).lit(16)
    data = g.bytes()
    for c in cuts:
        assert data[c:c + 2] == data[c - D1:c - D1 + 2] and data[c + 2] != data[c + 2 - D1] and data[c + 3:c + 32] == data[c + 3 - D1:c + 32 - D1]
    return ch.Built(data, [], cuts)


def expect_two_offsets_across_cuts(an, built, S, split=True):
    """split: the first sequence of each later segment is explicit, and the segment then uses Offset_Value 2 or 3 at least once (the
    rule of CZ_COMPRESS_SPLIT, which knows the top entry only, never writes those).  not split (the CZ_COMPRESS_HIGH frame of the same
    input): the first sequence behind each cut is a repeat code."""
    firsts = first_sequences(an, S)
    assert len(firsts) == 3 and all(blk["type"] == "compressed" for blk in an["blocks"])
    counts = check_history(an, S) if split else None
    for k in (1, 2):
        ll, ml, ofv = firsts[k]
        assert ll >= 3 and ml >= 29, (k, firsts[k])
        if split:
            assert ofv == D1 + 3, (k, firsts[k])
            assert counts[k][2] + counts[k][3] >= 1, (k, counts[k])
        else:
            assert ofv <= 3, (k, firsts[k])


def long_match_in_overlap(S, W):
    """compress_high.long_match_lost across a cut: 200 bytes that stand inside the last W bytes in front of the cut (F) start with
    four bytes that stand again, nearer and still in front of the cut, before other bytes (S); the 200 bytes stand again behind the
    cut.  The 4-byte table's one entry is S's, whether a block or the overlap insert put it there; only the second table still has
    F.  sites: [(p, position of F, position of S)]."""
    assert W >= 2048

    def build(seed):
        g = ce.Gen(seed).lit(S - 1500)
        f = len(g.b)
        g.lit(200)
        far = bytes(g.b[f:f + 200])
        g.lit(600)
        s = len(g.b)
        g.raw(far[:4]).lit(20)
        g.lit(S + 300 - len(g.b))
        p = len(g.b)
        g.raw(far).lit(16)
        data = g.bytes()
        c0 = p & ~(ch.CHUNK - 1)
        assert S - W <= f and s + 8 <= S < p and p - f <= W
        assert ch.nearest(data, p) == s and ch.match_len(data, p, s) < 8 and ch.match_len(data, p, f) == 200
        h = ch.hash8(data[p:p + 8])
        assert not any(ch.hash8(data[q:q + 8]) == h for q in range(f + 1, c0)), "the second table's entry is taken"
        return ch.Built(data, [(p, p - f, 200)], [(p, f, s)])
    return ch._seeded(build, 7000)


def sequence_at(an, p):
    """(ll, ml, offset) of the sequence whose match starts at input position p, or None."""
    for blk in an["blocks"]:
        pos = blk["start"]
        for (ll, ml, _), off in zip(blk["seqs"], blk.get("offsets", [])):
            pos += ll
            if pos == p:
                return ll, ml, off
            pos += ml
    return None


def expect_long_match_in_overlap(an, built, found=True):
    """found: a sequence of at least 200 bytes starts at the place with the far offset, so the second table was warmed from the
    overlap.  not found (CZ_COMPRESS_SPLIT | CZ_COMPRESS_FSE_TABLES on the same input): no such sequence."""
    ((p, f, _),) = built.sites
    got = sequence_at(an, p)
    if found:
        assert got is not None and got[1] >= 200 and got[2] == p - f, got
    else:
        assert got is None or not (got[1] >= 200 and got[2] == p - f), got
