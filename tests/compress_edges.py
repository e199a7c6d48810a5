"""Edge inputs of the zstd format for the compressor (cz_compress_frames_kernel), a full frame parser, and the references the edge
tests hold its frames to: the oracle's reading of each Huffman table and sequence, a Python model of the kernel's length-limited
Huffman build, and a package-merge routine that gives the optimal 11-bit-limited code.  Test infrastructure only.

Each edge input comes with a predicate on the analysed frame that says which branch of the encoder it must reach, so an input that
stops reaching its branch after a change fails instead of passing for nothing.  The inputs are rebuilt deterministically here; only
the sha256 of the frames is committed (tests/golden/compress_edges/manifest.json)."""
import random
from dataclasses import dataclass
from typing import Callable

import compress_frames as cf

KIB, MIB = 1 << 10, 1 << 20
BLOCK = 128 * KIB
WINDOW = MIB                    # the window of frames that are not single-segment
HUF_MAX_BITS = 11

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771,
                                65539]


def _code(bases, v):
    c = 0
    while c + 1 < len(bases) and bases[c + 1] <= v:
        c += 1
    return c


def ll_code(v):
    return _code(LL_BASE, v)


def ml_code(v):
    return _code(ML_BASE, v)


def of_code(offset_value):
    return offset_value.bit_length() - 1


def enc_hash(b4):
    """The encoder's hash of a 4-byte key (Knuth multiplicative, 14 bits)."""
    return ((int.from_bytes(b4, "little") * 2654435761) & 0xFFFFFFFF) >> 18


# ---------------------------------------------------------------------------------------------------------------- the frame parser
def _lit_header(body):
    b0 = body[0]
    lt, sf = b0 & 3, (b0 >> 2) & 3
    d = {"type": ("raw", "rle", "huffman", "treeless")[lt], "size_format": sf}
    if lt <= 1:
        hl = 1 if sf in (0, 2) else (2 if sf == 1 else 3)
        v = int.from_bytes(body[:hl], "little")
        d.update(header_len=hl, regen=v >> (3 if hl == 1 else 4), comp=None, streams=None)
        d["payload"] = d["regen"] if lt == 0 else 1
    else:
        hl = 3 if sf <= 1 else (4 if sf == 2 else 5)
        bits = 10 if hl == 3 else (14 if hl == 4 else 18)
        v = int.from_bytes(body[:hl], "little")
        d.update(header_len=hl, regen=(v >> 4) & ((1 << bits) - 1), comp=v >> (4 + bits), streams=1 if sf == 0 else 4)
        d["payload"] = d["comp"]
    return d


def _seq_header(body, at):
    b0 = body[at]
    if b0 < 128:
        n, hl = b0, 1
    elif b0 < 255:
        n, hl = ((b0 - 128) << 8) + body[at + 1], 2
    else:
        n, hl = body[at + 1] + (body[at + 2] << 8) + 0x7F00, 3
    return {"count": n, "header_len": hl, "modes": body[at + hl] if n else None}


def parse_frame(frame):
    """The frame header, and per block its type, size and (compressed blocks) literal and sequence section headers."""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    fhd = frame[4]
    fcs_flag, single, checksum, dict_flag = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
    pos = 5
    wd = None
    if not single:
        wd = frame[pos]
        pos += 1
    pos += (0, 1, 2, 4)[dict_flag]
    fcs_size = ((1 if single else 0), 2, 4, 8)[fcs_flag]
    fcs = int.from_bytes(frame[pos:pos + fcs_size], "little") + (256 if fcs_size == 2 else 0)
    pos += fcs_size
    if single:
        window = fcs
    else:
        base = 1 << (10 + (wd >> 3))
        window = base + (base >> 3) * (wd & 7)
    hdr = {"fcs_size": fcs_size, "single": single, "checksum": checksum, "content_size": fcs, "window": window, "header_len": pos}
    blocks = []
    while True:
        bh = int.from_bytes(frame[pos:pos + 3], "little")
        last, btype, size = bh & 1, (bh >> 1) & 3, bh >> 3
        t = ("raw", "rle", "compressed", "reserved")[btype]
        body = frame[pos + 3: pos + 3 + (1 if btype == 1 else size)]
        blk = {"type": t, "size": size, "at": pos, "body": body, "lit": None, "seq": None}
        if btype == 2:
            lit = _lit_header(body)
            if lit["type"] in ("huffman", "treeless"):
                lit["desc_form"] = None if lit["type"] == "treeless" else ("direct" if body[lit["header_len"]] >= 128 else "fse")
            blk["lit"] = lit
            blk["seq"] = _seq_header(body, lit["header_len"] + lit["payload"])
        blocks.append(blk)
        pos += 3 + len(body)
        if last:
            break
    return {"header": hdr, "blocks": blocks, "end": pos + (4 if checksum else 0)}


# ------------------------------------------------------------------------------------------------------------ Huffman references
def huf_model(hist):
    """The encoder's Huffman build restated: used symbols ranked by (count, symbol), a two-queue tree, depths cut to 11 bits and the
    Kraft sum repaired.  Returns (code length per symbol, tree depth before the cut)."""
    syms = sorted((c, s) for s, c in enumerate(hist) if c)
    n = len(syms)
    freq = [c for c, _ in syms]
    par = [0] * (2 * n)
    li, ni = 0, n
    for _ in range(n - 1):
        pick = []
        for _ in range(2):
            if li < n and (ni >= len(freq) or freq[li] <= freq[ni]):
                pick.append(li)
                li += 1
            else:
                pick.append(ni)
                ni += 1
        par[pick[0]] = par[pick[1]] = len(freq)
        freq.append(freq[pick[0]] + freq[pick[1]])
    depth = [0] * (2 * n - 1)
    for i in range(2 * n - 3, -1, -1):
        depth[i] = depth[par[i]] + 1
    deepest = max(depth[:n])
    cnt = [0] * (deepest + 2)
    for i in range(n):
        cnt[depth[i]] += 1
    cnt = cnt + [0] * max(0, HUF_MAX_BITS + 2 - len(cnt))
    for d in range(HUF_MAX_BITS + 1, len(cnt)):
        cnt[HUF_MAX_BITS] += cnt[d]
        cnt[d] = 0
    total = sum(cnt[d] << (HUF_MAX_BITS - d) for d in range(1, HUF_MAX_BITS + 1))
    while total > 1 << HUF_MAX_BITS:
        cnt[HUF_MAX_BITS] -= 1
        for d in range(HUF_MAX_BITS - 1, 0, -1):
            if cnt[d]:
                cnt[d] -= 1
                cnt[d + 1] += 2
                break
        total -= 1
    lengths, i = [0] * 256, n
    for d in range(1, HUF_MAX_BITS + 1):
        for _ in range(cnt[d]):
            i -= 1
            lengths[syms[i][1]] = d
    return lengths, deepest


def package_merge(hist, limit=HUF_MAX_BITS):
    """Optimal total code length (bits) of a prefix code for hist with no code longer than `limit` (package-merge)."""
    leaves = sorted((c, (s,)) for s, c in enumerate(hist) if c)
    if len(leaves) < 2:
        return sum(c for c, _ in leaves)
    assert len(leaves) <= 1 << limit
    cur = list(leaves)
    for _ in range(limit - 1):
        pk = [(cur[k][0] + cur[k + 1][0], cur[k][1] + cur[k + 1][1]) for k in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + pk, key=lambda x: x[0])
    length = [0] * 256
    for _, ss in cur[:2 * len(leaves) - 2]:
        for s in ss:
            length[s] += 1
    return sum(hist[s] * length[s] for s in range(256))


def weight_norm(lengths):
    """The FSE normalisation of the tree description the encoder starts from (weights of symbols 0 .. last-1, accuracy log 6):
    (number of weights, sum of the rounded probabilities before the repair, distinct weights)."""
    maxb = max(lengths)
    w = [maxb + 1 - l if l else 0 for l in lengths]
    last = max(s for s in range(256) if w[s])
    wc = [0] * 12
    for k in range(last):
        wc[w[k]] += 1
    norm = [max(1, c * 64 // last) if c else 0 for c in wc]
    return last, sum(norm), sum(1 for c in wc if c)


# -------------------------------------------------------------------------------------------------------------- frame analysis
def analyse(frame, data, dictionary=None):
    """parse_frame, plus per block: the sequences the oracle decodes (literal length, match length, Offset_Value, the actual
    offset), their LL / ML / OF codes, the block's literal bytes and histogram, and for Huffman literals the code lengths the oracle
    reads from the tree description.  dictionary: the raw dictionary the frame was written against; the offset history then starts
    from its three offsets, every offset must stay inside content + the data before the match, and the bytes each match copies are
    checked against content + data."""
    import oracle
    fr = parse_frame(frame)
    hist3, content = [1, 4, 8], b""
    if dictionary is None:
        st, seqs = oracle.dump_sequences(frame, cap=len(data) + 64)
    else:
        od = oracle.Dictionary(dictionary)
        assert od.status == 0, od.status
        st, seqs = oracle.dump_sequences(frame, cap=len(data) + 64, dictionary=od)
        hist3 = [od.info["hist0"], od.info["hist1"], od.info["hist2"]]
        content = bytes(dictionary)[od.info["content_off"]:]
    assert st == 0, st
    k, b0 = 0, 0
    D = len(content)
    for blk in fr["blocks"]:
        bsize = blk["size"]                                     # Raw and RLE blocks; a compressed block's from its sequences
        blk["seqs"] = []
        if blk["type"] == "compressed":
            n = blk["seq"]["count"]
            blk["seqs"] = seqs[k:k + n]
            k += n
            pos, lits, offs = b0, bytearray(), []
            for ll, ml, ofv in blk["seqs"]:
                if ofv > 3:
                    off = ofv - 3
                    hist3 = [off, hist3[0], hist3[1]]
                else:
                    r = ofv - (1 if ll else 0)            # 0 rep1, 1 rep2, 2 rep3, 3 rep1 - 1
                    off = hist3[0] - 1 if r == 3 else hist3[r]
                    if r == 1:
                        hist3 = [hist3[1], hist3[0], hist3[2]]
                    elif r >= 2:
                        hist3 = [off, hist3[0], hist3[1]]
                offs.append(off)
                lits += data[pos:pos + ll]
                pos += ll
                if dictionary is not None:
                    assert 0 < off <= D + pos, (off, D, pos)
                    _check_copy(content, data, pos, off, ml)
                pos += ml
            nlit_tail = blk["lit"]["regen"] - len(lits)         # the literals after the last sequence
            lits += data[pos:pos + nlit_tail]
            pos += nlit_tail
            blk["offsets"] = offs
            blk["literals"] = bytes(lits)
            bsize = pos - b0
        blk["start"] = b0
        b0 += bsize
        if blk["type"] == "compressed":
            h = [0] * 256
            for x in blk["literals"]:
                h[x] += 1
            blk["hist"] = h
            blk["ll_codes"] = {ll_code(ll) for ll, _, _ in blk["seqs"]}
            blk["ml_codes"] = {ml_code(ml) for _, ml, _ in blk["seqs"]}
            blk["of_codes"] = {of_code(o) for _, _, o in blk["seqs"]}
            lit = blk["lit"]
            if lit["type"] == "huffman":
                st, lengths, used = oracle.huf_code_lengths(blk["body"][lit["header_len"]:])
                assert st == 0, st
                lit["lengths"], lit["desc_len"] = lengths, used
    assert k == len(seqs) and b0 == len(data)
    return fr


def _check_copy(content, data, pos, off, ml):
    """The ml bytes a match at data[pos] with this offset copies, read from content + data, are data[pos:pos + ml]."""
    D, src = len(content), len(content) + pos - off                     # virtual position of the first byte copied
    n = min(ml, max(0, D - src))                                        # bytes that come from the content
    assert content[src:src + n] == data[pos:pos + n], (pos, off, ml)
    assert pos + ml <= len(data) and data[pos + n:pos + ml] == data[pos + n - off:pos + ml - off], (pos, off, ml)   # the rest from the data


# ---------------------------------------------------------------------------------------------------------------- input builders
class Gen:
    """Builds a byte string in which no 4-byte window repeats except inside copies appended on purpose: the encoder then finds the
    matches it is meant to find and no others (a hash collision can still hide one; the predicates check what was found)."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.b = bytearray()
        self.seen = set()

    def _push(self, x):
        self.b.append(x)
        if len(self.b) >= 4:
            self.seen.add(bytes(self.b[-4:]))

    def lit(self, n, alphabet=None, weights=None):
        alphabet = list(range(256)) if alphabet is None else list(alphabet)
        for _ in range(n):
            tail = bytes(self.b[-3:]) if len(self.b) >= 3 else None
            for _try in range(64):
                x = self.rng.choices(alphabet, weights)[0] if weights else self.rng.choice(alphabet)
                if tail is None or tail + bytes([x]) not in self.seen:
                    break
            else:
                x = next(x for x in self.rng.sample(alphabet, len(alphabet)) if tail + bytes([x]) not in self.seen)
            self._push(x)
        return self

    def exact(self, counts):
        """Literals with exactly counts[sym] of each symbol, in an order with no repeated 4-byte window."""
        for attempt in range(100):
            left = dict(counts)
            save_b, save_seen = bytearray(self.b), set(self.seen)
            ok = True
            for _ in range(sum(counts.values())):
                tail = bytes(self.b[-3:]) if len(self.b) >= 3 else None
                cand = [s for s, c in left.items() if c and (tail is None or tail + bytes([s]) not in self.seen)]
                if not cand:
                    ok = False
                    break
                x = self.rng.choices(cand, [left[s] for s in cand])[0]
                left[x] -= 1
                self._push(x)
            if ok:
                return self
            self.b, self.seen = save_b, save_seen
        raise RuntimeError("no order without repeated 4-byte windows")

    def copy(self, dist, n):
        for _ in range(n):
            self._push(self.b[-dist])
        return self

    def raw(self, bs):
        for x in bs:
            self._push(x)
        return self

    def bytes(self):
        return bytes(self.b)


def debruijn_tokens(length, seed=5):
    """K = 8 four-byte tokens with distinct first bytes in a cyclic de Bruijn order of degree 2, repeated: nearly every token is a
    4-byte match of its own, so a block holds up to about 32 760 sequences."""
    k, order = 8, 2
    a, seq = [0] * k * order, []

    def db(t, p):
        if t > order:
            if order % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    rng = random.Random(seed)
    toks = [bytes([0x41 + i]) + rng.randbytes(3) for i in range(k)]
    period = b"".join(toks[s] for s in seq)
    return (period * (length // len(period) + 1))[:length]


def mixed(n, seed, every=4096, copy=64, dist=2000, gen=False):
    """Unique literals with a copy of `copy` bytes from `dist` back every `every` bytes: compressed blocks with few sequences, all
    at one offset.  gen=True: the Gen, to go on from."""
    g = Gen(seed)
    while len(g.b) < n:
        g.lit(min(every - copy, n - len(g.b)))
        if len(g.b) + copy <= n and len(g.b) >= dist:
            g.copy(dist, copy)
    return g if gen else g.bytes()


def marked(n, mark_at, seed):
    """A 32-byte mark at 0, zeros (the encoder's hash table keeps the mark's entry: zeros add one key), the mark again at mark_at
    and unique non-zero bytes after it up to n."""
    rng = random.Random(seed)
    while True:
        mark = bytes(rng.randint(1, 255) for _ in range(32))
        keys = {bytes(mark[i:i + 4]) for i in range(29)}
        tailk = {(mark + b"\0\0\0")[i:i + 4] for i in range(29, 32)} | {b"\0\0\0\0"}
        if len(keys) == 29 and enc_hash(mark[:4]) not in {enc_hash(x) for x in (keys - {mark[:4]}) | tailk}:
            break
    b = bytearray(n)
    b[:32] = mark
    b[mark_at:mark_at + 32] = mark
    g = Gen(seed + 1)
    g.raw(b[mark_at - 3:mark_at + 32])
    g.lit(n - mark_at - 32, alphabet=range(1, 256))
    b[mark_at + 32:] = g.bytes()[35:]
    return bytes(b[:n])


def corpus_text(n):
    pool = b"".join(b for _, b in cf.corpus_originals())
    return pool[:n]


# ----------------------------------------------------------------------------------------------------------------- the edge list
@dataclass
class Edge:
    name: str
    data: bytes
    check: Callable             # check(analysed frame): asserts the branch the input is there to reach
    emu: bool = True            # small enough for the CPU emulator; False: the GPU test checks it against the oracle only
    raw_literals_ok: bool = False   # the encoder may keep Raw literals although a Huffman code would be smaller (see the check)


def _only(fr):
    assert len(fr["blocks"]) == 1, [b["type"] for b in fr["blocks"]]
    return fr["blocks"][0]


def _fcs(size, single):
    def chk(fr):
        assert fr["header"]["fcs_size"] == size and fr["header"]["single"] == single, fr["header"]
    return chk


def _lits(typ, hl, streams=None, form=None):
    def chk(fr):
        lit = _only(fr)["lit"]
        assert lit["type"] == typ and lit["header_len"] == hl, lit
        if streams:
            assert lit["streams"] == streams
        if form:
            assert lit["desc_form"] == form
    return chk


def _nseq(n, hl):
    def chk(fr):
        b = _only(fr)
        assert b["type"] == "compressed" and b["seq"]["count"] == n and b["seq"]["header_len"] == hl, b["seq"]
    return chk


def _raw_lit_input(nlit, seed):
    """nlit unique random literals, then a 16-byte copy of their last 16 (one sequence): a Raw literal section of exactly nlit."""
    return Gen(seed).lit(nlit).copy(16, 16).bytes()


def _skewed(n, seed, top=0x7A):
    """n literals, no repeated 4-byte window, 64 symbols up to `top` with falling weights: Huffman literals."""
    alpha = list(range(top - 63, top + 1))
    return Gen(seed).lit(n, alpha, [1.0 / (1 + i) ** 0.8 for i in range(64)]).bytes()


def _deep_counts(syms):
    """A Fibonacci chain (1, 1, 2, .. 55) under 20 symbols of count 89: the tree is 13 deep, cut to 11."""
    f = [1, 1]
    while len(f) < 10:
        f.append(f[-1] + f[-2])
    return dict(zip(syms, f + [89] * (len(syms) - 10)))


def _deep(fr, form):
    b = _only(fr)
    lit = b["lit"]
    assert lit["type"] == "huffman" and lit["desc_form"] == form, lit
    _, deepest = huf_model(b["hist"])
    assert deepest > HUF_MAX_BITS, deepest                               # the depth limit and the Kraft repair ran
    assert max(lit["lengths"]) == HUF_MAX_BITS


def _check_fse_parity(parity):
    def chk(fr):
        b = _only(fr)
        assert b["lit"]["desc_form"] == "fse"
        nw, _, _ = weight_norm(b["lit"]["lengths"])
        assert nw > 128 and nw % 2 == parity, nw
    return chk


def _window_exact(fr):
    assert not fr["header"]["single"] and fr["header"]["window"] == WINDOW
    last = fr["blocks"][-1]
    assert last["type"] == "compressed" and last["offsets"][0] == WINDOW and last["seqs"][0][0] == 0, last["seqs"]


def _window_plus1(fr):
    assert not fr["header"]["single"] and fr["header"]["window"] == WINDOW
    last = fr["blocks"][-1]
    assert last["type"] == "raw" and last["size"] == 65, "the mark 1 MiB + 1 back must stay literals"


def _rep_after_raw(fr):
    a, b, c = fr["blocks"]
    assert a["type"] == "compressed" and a["offsets"][-1] == 2000
    assert b["type"] == "raw"                                             # it had a sequence at offset 8 the decoder never sees
    (ll0, _, ofv0), (ll1, _, ofv1) = c["seqs"][:2]
    assert c["type"] == "compressed" and ll0 > 0 and ofv0 == 8 + 3        # not Offset_Value 1: the history is block A's
    assert ll1 > 0 and ofv1 == 1                                          # then a repeat offset


def _rep_across_rle(fr):
    a, z, c = fr["blocks"]
    assert a["type"] == "compressed" and a["offsets"][-1] == 2000 and z["type"] == "rle"
    assert c["type"] == "compressed" and c["seqs"][0][0] > 0 and c["seqs"][0][2] == 1 and c["offsets"][0] == 2000


def _rep_ll0_edge(fr):
    a, b = fr["blocks"]
    assert a["type"] == b["type"] == "compressed" and a["offsets"][-1] == 300
    ll, _, ofv = b["seqs"][0]
    assert ll == 0 and ofv == 300 + 3                                     # Offset_Value 1 would mean the second history entry


def _rle_lits2(fr):
    b = fr["blocks"][1]
    assert b["lit"]["type"] == "rle" and b["lit"]["regen"] == 2 and b["lit"]["header_len"] == 1, b["lit"]


def _huf_fallback(fr):
    b = _only(fr)
    assert b["type"] == "raw"
    lengths, _ = huf_model([b["body"].count(bytes([s])) for s in range(256)])
    nw, _, distinct = weight_norm(lengths)
    assert nw > 128 and distinct == 1, (nw, distinct)                    # one weight for all: no FSE description, Raw literals


def _multi(n_blocks, tail_type=None):
    def chk(fr):
        assert len(fr["blocks"]) == n_blocks, [b["type"] for b in fr["blocks"]]
        assert all(b["type"] == "compressed" for b in fr["blocks"][:-1] if b["size"] >= 16)
        if tail_type:
            assert fr["blocks"][-1]["type"] == tail_type, fr["blocks"][-1]["type"]
    return chk


def _codes_any(fr):
    assert any(b["seqs"] for b in fr["blocks"])


# sequence counts of de Bruijn inputs: debruijn_tokens(SEQ_LEN[n]) gives one block of exactly n sequences (measured on the emulator
# and asserted by the predicates)
SEQ_LEN = {127: 540, 128: 544, 129: 548, 0x7EFF: 130076, 0x7F00: 130080, 0x7F01: 130084}


def edges():
    """[Edge], deterministic."""
    E = []
    # sequence count: 1 / 2 / 3 header bytes
    for n in (127, 128, 129, 0x7EFF, 0x7F00, 0x7F01):
        E.append(Edge(f"seqs_{n:#x}", debruijn_tokens(SEQ_LEN[n]), _nseq(n, 1 if n < 128 else (2 if n < 0x7F00 else 3))))
    # Huffman: depth limit with FSE weights (odd and even count of weights), the direct / FSE boundary, one weight only
    for par, top in ((0, 234), (1, 235)):
        syms = [top - 7 * i for i in range(30)][::-1]
        E.append(Edge(f"huf_deep_fse_nw{top}", Gen(70 + par).exact(_deep_counts(syms)).bytes(),
                      lambda fr, par=par: (_deep(fr, "fse"), _check_fse_parity(par)(fr))))
    E.append(Edge("huf_deep_direct", Gen(72).exact(_deep_counts(list(range(0x41, 0x41 + 30)))).bytes(), lambda fr: _deep(fr, "direct")))
    E.append(Edge("huf_nw128_direct", _skewed(3000, 73, top=128), _lits("huffman", 4, 4, "direct")))
    E.append(Edge("huf_nw129_fse", _skewed(3000, 74, top=129), _lits("huffman", 4, 4, "fse")))
    E.append(Edge("huf_one_weight", Gen(75).exact({**{s: 16 for s in range(192)}, 192: 1024}).bytes(), _huf_fallback,
                  raw_literals_ok=True))
    # literal section headers: Raw 1 / 2 / 3 bytes, Huffman 3 / 4 / 5 bytes, RLE of two literals
    for n in (31, 32, 33, 4095, 4096, 4097):
        E.append(Edge(f"raw_lits_{n}", _raw_lit_input(n, 100 + n), _lits("raw", 1 if n < 32 else (2 if n < 4096 else 3))))
    for n in (1023, 1024, 1025, 16383, 16384, 16385):
        E.append(Edge(f"huf_lits_{n}", _skewed(n, 200 + n), _lits("huffman", 3 if n < 1024 else (4 if n < 16384 else 5),
                                                                   1 if n < 1024 else 4)))
    s = Gen(11).lit(40, alphabet=range(1, 254)).bytes()
    E.append(Edge("rle_lits_2", s + b"\x00" * (BLOCK - 40) + b"\xfe\xfe" + s, _rle_lits2))
    # frame header: Frame_Content_Size field and the single-segment flag
    for n in (255, 256, 257):
        E.append(Edge(f"fcs_{n}", mixed(n, n, every=64, copy=16, dist=40), _fcs(1 if n < 256 else 2, 1)))
    for n in (65791, 65792, 65793):
        E.append(Edge(f"fcs_{n}", mixed(n, n), _fcs(2 if n < 65792 else 4, 1)))
    for n, single in ((MIB - 1, 1), (MIB, 1), (MIB + 1, 0)):
        E.append(Edge(f"len_{n}", marked(n, n - 40, 12), _fcs(4, single)))
    # the window: a match exactly 1 MiB back is used, one 1 MiB + 1 back is not
    E.append(Edge("window_exact", marked(MIB + 64, MIB, 13), _window_exact))
    E.append(Edge("window_plus1", marked(MIB + 65, MIB + 1, 13), _window_plus1))
    # repeat offsets
    g = mixed(BLOCK, 21, gen=True)                                     # A: compressed, last offset 2000
    g.lit(5000).copy(8, 5).lit(BLOCK - 5005)                            # B: one 5-byte match at offset 8, worse than Raw
    g.lit(100).copy(8, 16).lit(100).copy(8, 16).lit(50)                 # C: offset 8 after literals, then again (repeat)
    E.append(Edge("rep_after_raw", g.bytes(), _rep_after_raw))
    g = mixed(BLOCK, 24, gen=True).raw(b"\x00" * BLOCK)               # A, then an RLE block
    g.lit(2500).copy(2000, 16).lit(400)                                 # offset 2000 after literals: Offset_Value 1
    E.append(Edge("rep_across_rle", g.bytes(), _rep_across_rle))
    g = Gen(25).raw(b"\x00" * (BLOCK - 400)).lit(360)                  # a match at offset 300 across the block boundary
    g.copy(300, 80).lit(100)
    E.append(Edge("rep_ll0_block_edge", g.bytes(), _rep_ll0_edge))
    # block counts at 128 KiB multiples and tails under 16 bytes
    for n, nb, tail in ((BLOCK - 1, 1, None), (BLOCK, 1, None), (BLOCK + 1, 2, "rle"), (BLOCK + 15, 2, "raw"), (BLOCK + 16, 2, None),
                        (2 * BLOCK - 1, 2, None), (2 * BLOCK + 1, 3, "rle"), (2 * BLOCK + 7, 3, "raw")):
        E.append(Edge(f"blocks_{n}", mixed(n, 30 + n % 97), _multi(nb, tail)))
    # LL / ML codes: a ladder of literal runs and match lengths through every code's lowest value
    E += code_ladders()
    E.append(Edge("offsets", offset_ladder(), _offsets))
    E.append(Edge("text", corpus_text(24000), _codes_any))
    # larger than the emulator can take in the time the CPU tests have: a 2.1 MiB input with matches exactly 1 MiB back
    E.append(Edge("big_window_exact", big_window(), _big_window, emu=False))
    return E


def code_ladders():
    """Inputs whose sequences run through the lowest value of every LL code from 4 and every ML code from 1 (length 4): literal run
    L then a match of length M at a short offset (a period copy of the run's end)."""
    lls = [LL_BASE[c] for c in range(4, 36)]
    mls = [ML_BASE[c] for c in range(1, 53)]
    pairs = [(lls[i] if i < len(lls) else 8, mls[i] if i < len(mls) else 4) for i in range(max(len(lls), len(mls)))]
    pairs.sort(key=lambda p: p[0] + p[1])
    out, cur, size = [], [], 0
    for p in pairs:                                                     # pack into single-block inputs
        if size + p[0] + p[1] + 64 > BLOCK - 64:
            out.append(cur)
            cur, size = [], 0
        cur.append(p)
        size += p[0] + p[1] + 8
    out.append(cur)
    E = []
    for k, group in enumerate(out):
        g = Gen(300 + k)
        for ll, ml in group:
            g.lit(ll)
            g.copy(min(ll, 8), ml)
        g.lit(8)
        want_ll = {ll_code(ll) for ll, _ in group}
        want_ml = {ml_code(ml) for _, ml in group}

        def chk(fr, want_ll=want_ll, want_ml=want_ml):
            got_ll = set().union(*(b.get("ll_codes", set()) for b in fr["blocks"]))
            got_ml = set().union(*(b.get("ml_codes", set()) for b in fr["blocks"]))
            assert want_ll <= got_ll and want_ml <= got_ml, (sorted(want_ll - got_ll), sorted(want_ml - got_ml))
        E.append(Edge(f"codes_{k}", g.bytes(), chk))
    return E


OFFSET_LADDER = range(8, 20)


def offset_ladder(seed=15):
    """Zeros with 16-byte marks, each again 3 * 2^(k-1) - 3 bytes later (Offset_Value in the middle of OF code k): the encoder's
    hash table holds little more than the marks, so every second copy finds its first."""
    rng = random.Random(seed)
    pos = {k: (64 + 32 * (k - 8), 64 + 32 * (k - 8) + 3 * (1 << (k - 1)) - 3) for k in OFFSET_LADDER}
    b = bytearray(max(y for _, y in pos.values()) + 64)
    for k, (x, y) in pos.items():
        m = bytes(rng.randint(1, 255) for _ in range(16))
        b[x:x + 16] = m
        b[y:y + 16] = m
    return bytes(b)


def _offsets(fr):
    got = {of_code(o) for b in fr["blocks"] if b["type"] == "compressed" for _, _, o in b["seqs"]}
    assert set(OFFSET_LADDER) <= got, sorted(set(OFFSET_LADDER) - got)


def big_window():
    """2.1 MiB: text, a mark, zeros, the mark again exactly 1 MiB later, text."""
    text = corpus_text(BLOCK)
    m = marked(MIB + 200, MIB, 14)
    body = text + m[:MIB + 64] + text[::-1] * 8
    return body[:2 * MIB + 100 * KIB]


def _big_window(fr):
    assert not fr["header"]["single"]
    assert WINDOW in {o for b in fr["blocks"] if b["type"] == "compressed" for o in b["offsets"]}
    assert all(o <= WINDOW for b in fr["blocks"] if b["type"] == "compressed" for o in b["offsets"])


def emu_edges():
    return [e for e in edges() if e.emu]
