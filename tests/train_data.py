"""Inputs of the dictionary training tests and a reader of a dictionary's header that shares no code with the kernels (RFC 8878
§4.1.1 FSE table descriptions, §4.2.1 Huffman tree descriptions, §5 dictionary format).  Test infrastructure only."""
import numpy as np

import dict_records as dr

MAGIC = 0xEC30A437
PLANT_LEN = 64


def _planted(seed, plants, hits, n=64, size=1024):
    """n samples of `size` seeded random bytes; plants[k] is written over sample i when i is in hits[k] (places never overlap)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        b = bytearray(rng.integers(0, 256, size, dtype=np.uint8).tobytes())
        slots = rng.permutation(size // 128)                             # one 128-byte slot per string
        for k, p in enumerate(plants):
            at = int(slots[k]) * 128 + int(rng.integers(0, 128 - len(p)))
            if i in hits[k]:
                b[at:at + len(p)] = p
        out.append(bytes(b))
    return out


def planted():
    """Case 1: (samples, the string every sample holds once)."""
    s = bytes(np.random.default_rng(11).integers(0, 256, PLANT_LEN, dtype=np.uint8))
    return _planted(12, [s], [set(range(64))]), s


def two_planted():
    """Case 2: (samples, the string in 58 of them, the string in 19 of them)."""
    rng = np.random.default_rng(21)
    a, b = (bytes(rng.integers(0, 256, PLANT_LEN, dtype=np.uint8)) for _ in range(2))
    order = [int(x) for x in rng.permutation(64)]
    return _planted(22, [a, b], [set(order[:58]), set(order[40:59])]), a, b


def family_records(j, n, seed=None):
    """n training records of family j (seed 1000 + j unless given): not the held-out records of dict_records.records."""
    rng = np.random.default_rng(1000 + j if seed is None else seed)
    return [dr.record(dr.FAMILIES[j][0], rng, i) for i in range(n)]


def manifest_inputs():
    """{name: (samples, capacity)} of tests/golden/train/manifest.json (scripts/gen_train_manifest.py)."""
    return {"planted": (planted()[0], 2048), "two_planted": (two_planted()[0], 2048), "users150": (family_records(0, 150), 2048)}


# ------------------------------------------------------------------ reading a dictionary
def _ncount(data, pos, max_log):
    """FSE table description at data[pos:]: (probabilities with -1 for 'less than 1', accuracy log, position behind it)."""
    acc, nb, at = 0, 0, pos

    def read(n):
        nonlocal acc, nb, at
        while nb < n:
            acc |= data[at] << nb
            at += 1
            nb += 8
        v = acc & ((1 << n) - 1)
        acc >>= n
        nb -= n
        return v

    def unread(n, v):
        nonlocal acc, nb
        acc = (acc << n) | v
        nb += n

    log = 5 + read(4)
    assert log <= max_log, (log, max_log)
    remaining, probs = 1 << log, []
    while remaining > 0:
        bits = (remaining + 1).bit_length()
        low = (1 << bits) - 1 - (remaining + 1)
        mask = (1 << (bits - 1)) - 1
        v = read(bits)
        if (v & mask) < low:
            unread(1, v >> (bits - 1))
            v &= mask
        elif v > mask:
            v -= low
        p = v - 1
        probs.append(p)
        remaining -= 1 if p == -1 else p
        assert remaining >= 0
        if p == 0:
            while True:
                r = read(2)
                probs += [0] * r
                if r != 3:
                    break
    return probs, log, at - nb // 8


def _fse_table(probs, log):
    size = 1 << log
    sym, high = [0] * size, size - 1
    for s, p in enumerate(probs):
        if p == -1:
            sym[high] = s
            high -= 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, p in enumerate(probs):
        for _ in range(max(p, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    nxt = [1 if p == -1 else p for p in probs]
    table = []
    for u in range(size):
        x = nxt[sym[u]]
        nxt[sym[u]] += 1
        n = log - (x.bit_length() - 1)
        table.append((sym[u], n, (x << n) - size))
    return table


def _huffman_weights(data, pos):
    """Huffman tree description at data[pos:]: (the weights of all symbols, the last one derived; position behind it)."""
    hb = data[pos]
    if hb >= 128:
        n = hb - 127
        raw = data[pos + 1: pos + 1 + (n + 1) // 2]
        w = [(raw[k // 2] >> (4 if k % 2 == 0 else 0)) & 15 for k in range(n)]
        end = pos + 1 + (n + 1) // 2
    else:
        probs, log, at = _ncount(data, pos + 1, 6)
        table = _fse_table(probs, log)
        stream = data[at: pos + 1 + hb]
        assert stream and stream[-1]
        value = int.from_bytes(stream, "little")
        left = len(stream) * 8 - (8 - stream[-1].bit_length()) - 1      # bits below the closing 1

        def read(n):
            nonlocal left
            left -= n
            if left >= 0:
                return (value >> left) & ((1 << n) - 1)
            return ((value << -left) & ((1 << n) - 1)) if n + left > 0 else 0   # past the start: zeros

        s1, s2, w = read(log), read(log), []
        assert left >= 0
        while True:
            w.append(table[s1][0])
            s1 = table[s1][2] + read(table[s1][1])
            if left < 0:
                w.append(table[s2][0])
                break
            w.append(table[s2][0])
            s2 = table[s2][2] + read(table[s2][1])
            if left < 0:
                w.append(table[s1][0])
                break
        end = pos + 1 + hb
    total = sum(1 << (x - 1) for x in w if x)
    top = 1 << total.bit_length()                                        # the next power of two above the sum
    rest = top - total
    assert rest & (rest - 1) == 0, "the last weight is no power of two"
    return w + [rest.bit_length()], end


def parse(raw):
    """The fields of a dictionary: magic, id, weights (per literal value), max_bits, of / ml / ll = (probabilities, log), rep,
    content."""
    raw = bytes(raw)
    out = {"magic": int.from_bytes(raw[0:4], "little"), "id": int.from_bytes(raw[4:8], "little")}
    w, at = _huffman_weights(raw, 8)
    out["weights"] = w
    out["max_bits"] = sum(1 << (x - 1) for x in w if x).bit_length() - 1
    for name, max_log in (("of", 8), ("ml", 9), ("ll", 9)):
        probs, log, at = _ncount(raw, at, max_log)
        out[name] = (probs, log)
    out["rep"] = [int.from_bytes(raw[at + 4 * k: at + 4 * k + 4], "little") for k in range(3)]
    out["content"] = raw[at + 12:]
    return out


def check_valid(raw, capacity, dict_id=None):
    """Everything a trained dictionary promises, from its bytes alone; returns parse(raw)."""
    import oracle
    assert len(raw) <= capacity
    d = parse(raw)
    assert d["magic"] == MAGIC
    assert d["rep"] == [1, 4, 8] and len(d["content"]) >= 8
    want = dict_id if dict_id else 32768 + oracle.xxh64(d["content"]) % ((1 << 31) - 32768)
    assert d["id"] == want
    assert len(d["weights"]) == 256 and all(d["weights"]) and d["max_bits"] <= 11
    for name, codes, max_log in (("ll", 36, 9), ("ml", 53, 9), ("of", 21, 8)):
        probs, log = d[name]
        assert log <= max_log and len(probs) >= codes and all(p != 0 for p in probs[:codes]), name
        assert len(probs) <= (32 if name == "of" else codes)
    od = oracle.Dictionary(raw)
    assert od.status == 0 and od.info["id"] == d["id"] and od.info["content_len"] == len(d["content"])
    assert [od.info["hist0"], od.info["hist1"], od.info["hist2"]] == [1, 4, 8]
    return d
