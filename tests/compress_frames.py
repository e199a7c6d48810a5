"""Helpers of the compression tests: a walk over the blocks of a frame (block types, literal section types, Huffman stream count and
tree description form), libzstd when the host has it, and the inputs the tests share.  Test infrastructure only."""
import ctypes
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = os.path.join(ROOT, "tests", "golden", "decode_corpus")


def corpus_originals(max_len=None):
    out = []
    for n in sorted(os.listdir(CORPUS)):
        if n.endswith(".zst"):
            continue
        b = open(os.path.join(CORPUS, n), "rb").read()
        if max_len is None or len(b) <= max_len:
            out.append((n, b))
    return out


def walk(frame):
    """[(block type, info)] — info for compressed blocks: dict(lit=literal type, streams, desc='direct'|'fse'|None)."""
    fhd = frame[4]
    fcs_flag, single, dict_flag = fhd >> 6, (fhd >> 5) & 1, fhd & 3
    pos = 5 + (0 if single else 1) + (0, 1, 2, 4)[dict_flag] + ((1 if single else 0), 2, 4, 8)[fcs_flag]
    blocks = []
    while True:
        bh = int.from_bytes(frame[pos:pos + 3], "little")
        last, btype, size = bh & 1, (bh >> 1) & 3, bh >> 3
        body = frame[pos + 3: pos + 3 + (1 if btype == 1 else size)]
        info = {}
        if btype == 2:
            lt, sf = body[0] & 3, (body[0] >> 2) & 3
            info["lit"] = ("raw", "rle", "huffman", "treeless")[lt]
            if lt == 2:
                info["streams"] = 1 if sf == 0 else 4
                hdr = 3 if sf < 2 else (4 if sf == 2 else 5)
                info["desc"] = "direct" if body[hdr] >= 128 else "fse"
        blocks.append((("raw", "rle", "compressed", "reserved")[btype], info))
        pos += 3 + len(body)
        if last:
            break
    return blocks


_zstd = None


def libzstd():
    """libzstd.so.1 through ctypes, or None."""
    global _zstd
    if _zstd is None:
        try:
            z = ctypes.CDLL("libzstd.so.1")
            z.ZSTD_decompress.restype = ctypes.c_size_t
            z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
            z.ZSTD_isError.restype = ctypes.c_uint
            z.ZSTD_isError.argtypes = [ctypes.c_size_t]
            _zstd = z
        except OSError:
            _zstd = False
    return _zstd or None


def libzstd_decompress(frame, n):
    z = libzstd()
    out = ctypes.create_string_buffer(n + 1)
    src = ctypes.create_string_buffer(bytes(frame), len(frame))
    r = z.ZSTD_decompress(out, n + 1, src, len(frame))
    return None if z.ZSTD_isError(r) else out.raw[:r]


def special_inputs():
    """name -> bytes: the edge cases of the frame format the encoder pins."""
    rng = random.Random(1234)
    words = [bytes(rng.choice(b"etaoinshrdlucmfwyp") for _ in range(rng.randint(2, 9))) for _ in range(300)]
    text = b" ".join(rng.choice(words) for _ in range(900))           # largest byte < 128: direct weights
    allbytes = bytes(range(256)) + bytes(rng.choices(range(256), weights=[1.0 / (1 + (i * 37) % 256) for i in range(256)], k=4000))
    return {
        "empty": b"", "one": b"A", "three": b"xyz",
        "rle64k": b"\x5c" * 65536,
        "random64k": rng.randbytes(65536),
        "text_ascii": text,
        "all_bytes": allbytes,
        "lit_under_1k": bytes(rng.choice(b"abcdefgh") for _ in range(1500)),
        "lit_over_1k": bytes(rng.choice(b"abcdefgh") for _ in range(1900)),
        "long_match": b"hd" + b"\xa7" * 70000 + b"tail",
    }
