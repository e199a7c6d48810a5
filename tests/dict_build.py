"""A writer of zstd dictionaries (RFC 8878 §5): magic, Dictionary_ID, a Huffman tree description, the OF / ML / LL FSE table
descriptions (§4.1.1), three repeat offsets and the content.  It shares no code with the kernels and is the exact inverse of the
reader in train_data (parse, _ncount, _huffman_weights).  Test infrastructure only."""
MAGIC = 0xEC30A437


class _Bits:
    """Little-endian bit writer: the first value written lands in the lowest bits of the first byte."""

    def __init__(self):
        self.acc, self.nb = 0, 0

    def add(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.nb
        self.nb += n

    def bytes(self):
        return self.acc.to_bytes((self.nb + 7) // 8, "little")


def ncount(probs, log):
    """The FSE table description of `probs` (-1: 'less than 1') at accuracy log `log`.  The last probability is not 0."""
    assert 5 <= log <= 9 and probs and probs[-1] != 0
    assert sum(1 if p == -1 else p for p in probs) == 1 << log, (sum(1 if p == -1 else p for p in probs), log)
    w = _Bits()
    w.add(log - 5, 4)
    remaining, s = 1 << log, 0
    while s < len(probs):
        p = probs[s]
        assert p >= -1 and remaining > 0
        bits = (remaining + 1).bit_length()
        low = (1 << bits) - 1 - (remaining + 1)                          # values below it take one bit less
        mask = (1 << (bits - 1)) - 1
        value = p + 1
        if value < low:
            w.add(value, bits - 1)
        else:
            w.add(value + low if value > mask else value, bits)
        remaining -= 1 if p == -1 else p
        s += 1
        if p == 0:                                                       # how many more zeros follow, 2 bits at a time (3: go on)
            z = 0
            while probs[s + z] == 0:
                z += 1
            s += z
            while z >= 3:
                w.add(3, 2)
                z -= 3
            w.add(z, 2)
    assert remaining == 0
    return w.bytes()


def huffman_direct(weights):
    """The direct form of a Huffman tree description: at most 128 weights of 4 bits; the weight of the next symbol is implied."""
    n = len(weights)
    assert 1 <= n <= 128 and all(0 <= x <= 11 for x in weights)
    total = sum(1 << (x - 1) for x in weights if x)
    rest = (1 << total.bit_length()) - total
    assert rest & (rest - 1) == 0, "the implied last weight is no power of two"
    out = bytearray([127 + n])
    for k in range(0, n, 2):
        out.append((weights[k] << 4) | (weights[k + 1] if k + 1 < n else 0))
    return bytes(out)


def build(dict_id, huf, of, ml, ll, rep, content):
    """The dictionary's bytes.  huf: a list of weights (direct form) or ready-made description bytes; of / ml / ll:
    (probabilities, accuracy log); rep: three offsets; content: bytes."""
    out = bytearray(MAGIC.to_bytes(4, "little") + int(dict_id).to_bytes(4, "little"))
    out += bytes(huf) if isinstance(huf, (bytes, bytearray)) else huffman_direct(list(huf))
    for probs, log in (of, ml, ll):
        out += ncount(list(probs), log)
    assert len(rep) == 3
    for r in rep:
        out += int(r).to_bytes(4, "little")
    return bytes(out + bytes(content))


# Dictionaries of dict_edges that libzstd refuses to load, with the reason.  Only dictionaries of the "content sizes" group.
LIBZSTD_REFUSES = {
    "content_0": "a repeat offset larger than the content (0 bytes)",
    "content_3": "a repeat offset larger than the content (3 bytes)",
}

# Dictionaries of dict_edges that libzstd's compressor refuses although its decoder loads them, with the reason.  test_dict_build
# gives libzstd's decoder a frame compressed with the bare content as a raw-content dictionary instead.
LIBZSTD_COMPRESSOR_REFUSES = {
    "huf_direct": "its compressor wants a Huffman code for all 256 symbols; this one has 129",
}
