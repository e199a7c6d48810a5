"""Helpers of the CZ_COMPRESS_FSE_TABLES tests: a walker that reads each Compressed block's Compression_Modes byte and its FSE table
descriptions (RFC 8878 §4.1.1, restated here: it shares no code with the kernel), and the inputs that steer the encoder to each mode
and each form of the description.  Test infrastructure only."""
import random

import compress_edges as ce
import compress_frames as cf

PREDEFINED, RLE, FSE = 0, 1, 2
MAX_LOG = {"ll": 9, "of": 8, "ml": 9}
MAX_SYM = {"ll": 35, "of": 31, "ml": 52}


def read_table(buf, at, field):
    """One FSE table description at buf[at:]: dict(log, probs (-1: less than 1), flags (the 2-bit zero-repeat flags read), short (values
    read in the short form), len (bytes))."""
    pos = 0

    def bits(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= ((buf[at + ((pos + i) >> 3)] >> ((pos + i) & 7)) & 1) << i
        pos += n
        return v
    log = bits(4) + 5
    assert 5 <= log <= MAX_LOG[field], (field, log)
    remaining, probs, flags, short = 1 << log, [], [], 0
    while remaining > 0:
        max_rem = remaining + 1
        nb = max_rem.bit_length()
        low = (1 << nb) - 1 - max_rem
        v = bits(nb - 1)
        if v < low:
            short += 1
        else:
            v |= bits(1) << (nb - 1)
            if v >= 1 << (nb - 1):
                v -= low
        p = v - 1
        probs.append(p)
        remaining -= 1 if p == -1 else p
        assert remaining >= 0, field
        if p == 0:
            while True:
                r = bits(2)
                flags.append(r)
                probs += [0] * r
                if r != 3:
                    break
    assert len(probs) - 1 <= MAX_SYM[field], (field, len(probs))
    assert sum(1 if p == -1 else p for p in probs) == 1 << log
    assert sum(1 for p in probs if p) >= 2, "a one-symbol table must be RLE_Mode"
    return {"log": log, "probs": probs, "flags": flags, "short": short, "len": (pos + 7) >> 3}


def modes(frame):
    """Per Compressed block with sequences: dict(nseq, ll / of / ml = mode, tables = {field: read_table(...)}, rle = {field: symbol})."""
    out = []
    for blk in ce.parse_frame(frame)["blocks"]:
        if blk["type"] != "compressed" or not blk["seq"]["count"]:
            continue
        body, lit, seq = blk["body"], blk["lit"], blk["seq"]
        at = lit["header_len"] + lit["payload"] + seq["header_len"]
        m = body[at]
        assert m & 3 == 0, "reserved bits of Compression_Modes"
        d = {"nseq": seq["count"], "ll": m >> 6, "of": (m >> 4) & 3, "ml": (m >> 2) & 3, "tables": {}, "rle": {}}
        at += 1
        for f in ("ll", "of", "ml"):
            assert d[f] != 3, "Repeat_Mode is never written"
            if d[f] == RLE:
                d["rle"][f] = body[at]
                at += 1
            elif d[f] == FSE:
                d["tables"][f] = read_table(body, at, f)
                at += d["tables"][f]["len"]
        out.append(d)
    return out


def same_block_types(a, b):
    return [t for t, _ in cf.walk(a)] == [t for t, _ in cf.walk(b)]


# ----------------------------------------------------------------------------------------------------------------------- inputs
def one_sequence():
    return ce.Gen(401).lit(50).copy(20, 10).lit(30).bytes()


def two_sequences():
    """Two sequences that differ in every code (LL 300 / 7, ML 10 / 16, distances 20 / 200): no field can be RLE."""
    return ce.Gen(402).lit(300).copy(20, 10).lit(7).copy(200, 16).lit(30).bytes()


def runs_and_copies(steps, seed):
    """steps = [(L, M, j)]: L never-repeating literals, then M bytes copied from the start of the literal run j steps back (j = 0: this
    step's own; no copy while there is no such run).  Every source is a literal run that is copied from once or a few times at
    different distances, so the parse finds the copy as one match, a byte or two late at worst (a hash collision); a copy never
    has the distance of the copy before it, so no offset is written as a repeat."""
    g = ce.Gen(seed)
    starts, prev = [], None
    for k, (L, M, j) in enumerate(steps):
        starts.append(len(g.b))
        g.lit(L)
        if k - j < 0:
            continue
        assert steps[k - j][0] > M
        dist = len(g.b) - starts[k - j]
        if dist == prev:
            dist -= 1
        g.copy(dist, M)
        prev = dist
    g.lit(20)
    return g.bytes()


def fixed_copies(n=300, seed=403):
    """Copies of 62 bytes (the middle of ML code 39: 59 to 66) from 9 steps back (1 188 to 1 228 bytes: OF code 10, 1 021 to 2 044)
    behind 63 to 67 literals (LL codes 24 and 25): one OF code, one ML code, several LL codes.  The first nine runs, which have
    nothing to copy from, are twice as long, so that the first copies reach as far back as the later ones."""
    rng = random.Random(seed)
    return runs_and_copies([(130 if k < 9 else rng.randint(63, 67), 62, 9) for k in range(n)], seed)


def skewed_ml(n=800, seed=404):
    """Match length 62 (ML code 39) in all but seven of 800 sequences; seven other lengths once each."""
    rng = random.Random(seed)
    once = {100 + 90 * i: m for i, m in enumerate((20, 25, 30, 36, 40, 45, 52))}
    return runs_and_copies([(rng.randint(63, 70), once.get(k, 62), 8) for k in range(n)], seed)


def gapped_codes(n=600, seed=405):
    """44 bytes alternately from this step's own 45 to 51 literals (OF code 5) and from 60 steps back (about 5 600 bytes: OF code 12):
    five unused OF codes in front of the first used one, six between the two."""
    rng = random.Random(seed)
    return runs_and_copies([(rng.randint(45, 51), 44, 60 if k % 2 and k > 60 else 0) for k in range(n)], seed)


def many_ml_codes(seed=406):
    """ML codes 10 to 44, each once, and code 40 (match lengths 67 to 82) 90 more times: 35 codes in a block of fewer than 256
    sequences, whose accuracy log would be 5 by the sequence count.  Every source lies 256 bytes back or more (an earlier chunk)."""
    rng = random.Random(seed)
    mls = [ce.ML_BASE[c] for c in range(10, 45)] + [75] * 90
    rng.shuffle(mls)
    return runs_and_copies([(max(m + 1, 131) + rng.randint(0, 4), m, 1 if m <= 130 else 0) for m in mls], seed)


def far_offsets(seed=407):
    """Two blocks: 3 000 unique bytes, 150 KiB of zeros, then 400 copies alternately from the unique bytes (more than 128 KiB back:
    OF code 17) and from 600 / 900 bytes back."""
    g = ce.Gen(seed)
    rng = random.Random(seed)
    g.lit(3000, alphabet=range(1, 256))
    g.raw(b"\x00" * (150 << 10))
    g.lit(1500, alphabet=range(1, 256))
    for k in range(400):
        g.lit(rng.randint(2, 8), alphabet=range(1, 256))
        if k % 2:
            g.copy((600, 900)[(k >> 1) & 1], 8)
        else:
            g.copy(len(g.b) - (100 + 6 * k), 8)
    g.lit(20, alphabet=range(1, 256))
    return g.bytes()
