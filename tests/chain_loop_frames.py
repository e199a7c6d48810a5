"""Batches for the tests of cz_chain_kernel's main loop (test_chain_loop_gpu.py on the device, test_emu_chain_loop.py on the CPU
emulator): slots of one wave that use up their bit rings at very different rates, bitstreams at every byte alignment, slots that
take block after block.  A wave's ten owner lanes take blocks off one list, so a few dozen blocks already put live slots with
different needs into the same wave."""
import ctypes

import numpy as np

import oracle
from cairo_zstd_amd import synth


def walk_blocks(fr: bytes):
    """[(block type, offset of the block's body in the frame, bytes of the body)] of a frame, and the offset behind its last block."""
    d = fr[4]
    fcs, single, did = d >> 6, (d >> 5) & 1, d & 3
    p = 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0) if fcs == 0 else (2, 4, 8)[fcs - 1])
    blocks = []
    while True:
        h = int.from_bytes(fr[p:p + 3], "little")
        t, size = (h >> 1) & 3, h >> 3
        body = 1 if t == 1 else size
        blocks.append((t, p + 3, body))
        p += 3 + body
        if h & 1:
            return blocks, p


def libzstd():
    try:
        L = ctypes.CDLL("libzstd.so.1")
    except OSError:
        return None
    L.ZSTD_compress.restype = ctypes.c_size_t
    L.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    L.ZSTD_isError.restype = ctypes.c_uint
    L.ZSTD_isError.argtypes = [ctypes.c_size_t]
    L.ZSTD_compressBound.restype = ctypes.c_size_t
    L.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    return L


def _compress(L, d: bytes, level: int) -> bytes:
    cap = L.ZSTD_compressBound(len(d))
    dst = ctypes.create_string_buffer(cap)
    n = L.ZSTD_compress(dst, cap, d, len(d), level)
    assert not L.ZSTD_isError(n)
    return dst.raw[:n]


def long_match_long_literal_data(rng, size: int, far_lo: int = 600_000, far_hi: int = 1_200_000) -> bytes:
    """Text-like stretches (thousands of short sequences per block, so the blocks run through the groups of 32 steps) with, every
    few ten KB, a run of noise of 5 .. 20 KB and a copy of 3 .. 20 KB of noise from far_lo .. far_hi bytes (0.6 .. 1.2 MB) further up: sequences with a
    long literal run, a long match and a far offset at once, more than 32 extra bits together, in the middle of ordinary ones."""
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(400)]
    out = bytearray()
    noise_at = []                                                       # (position, length) of the runs of noise so far
    while len(out) < size:
        out += b" ".join(words[int(i)] for i in rng.integers(0, len(words), int(rng.integers(2000, 9000))))
        n = int(rng.integers(5000, 20000))
        noise_at.append((len(out), n))
        out += rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        far = [(p, ln) for p, ln in noise_at if far_lo <= len(out) - p <= far_hi and ln >= 3000]
        if far:
            p, ln = far[int(rng.integers(0, len(far)))]
            out += out[p:p + min(ln, int(rng.integers(3000, 20000)))]
    return bytes(out[:size])


def mixed_rates(n_each: int, small: bool = False):
    """(frames, capacities): config 4a frames (about 15 bits per sequence: a top-up every fourth group), `mix` frames and — with
    a libzstd on the box — long-match / long-literal frames (a top-up nearly every group, the wide redo right behind one),
    interleaved so that neighbouring blocks of the list, hence the slots of one wave, are of different kinds.
    small: what the CPU emulator gets through in seconds — no config 4a frame (32 768 sequences are a minute there), mix frames
    below 40 KB, 100 KB of long-match data with the far copies 30 .. 60 KB up."""
    m = synth.generate("mix", 8 * n_each if small else n_each, first_index=7300, nthreads=2)
    keep = [i for i in range(m.n) if 2000 < m.regen[i] < 40000][:n_each] if small else list(range(n_each))
    kinds = [[(m.frame(i), int(m.regen[i])) for i in keep]]
    if not small:
        a = synth.generate("full_4a", n_each, first_index=5100, nthreads=2)
        kinds.insert(0, [(a.frame(i), int(a.regen[i])) for i in range(n_each)])
    L = libzstd()
    if L is not None:
        rng = np.random.default_rng(31)
        real = []
        for i in range(n_each):
            d = long_match_long_literal_data(rng, 100_000, 30_000, 60_000) if small else long_match_long_literal_data(rng, int(rng.integers(900_000, 1_500_000)))
            real.append((_compress(L, d, (3, 9)[i % 2]), len(d)))
        kinds.append(real)
    frames, caps = [], []
    for i in range(n_each):
        for k in kinds:
            if i < len(k):
                frames.append(k[i][0])
                caps.append(k[i][1])
    return frames, caps


def many_small_blocks(L, n_frames: int, blocks_per_frame: int, seed: int = 5):
    """Frames of `blocks_per_frame` compressed blocks of about 2 KB of text each (libzstd ends a block at every flush): far more
    blocks with sequences than a launch has slots, each long enough for several groups of 32 steps."""
    class Buf(ctypes.Structure):
        _fields_ = [("p", ctypes.c_void_p), ("size", ctypes.c_size_t), ("pos", ctypes.c_size_t)]
    L.ZSTD_createCCtx.restype = ctypes.c_void_p
    L.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
    L.ZSTD_compressStream2.restype = ctypes.c_size_t
    L.ZSTD_compressStream2.argtypes = [ctypes.c_void_p, ctypes.POINTER(Buf), ctypes.POINTER(Buf), ctypes.c_int]
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(250)]
    frames, caps = [], []
    for _ in range(n_frames):
        cctx = L.ZSTD_createCCtx()
        dst = ctypes.create_string_buffer(8192 * blocks_per_frame)
        ob = Buf(ctypes.cast(dst, ctypes.c_void_p), len(dst), 0)
        total = 0
        for b in range(blocks_per_frame):
            chunk = b" ".join(words[int(i)] for i in rng.integers(0, len(words), int(rng.integers(300, 500))))
            src = ctypes.create_string_buffer(chunk, len(chunk))
            ib = Buf(ctypes.cast(src, ctypes.c_void_p), len(chunk), 0)
            r = L.ZSTD_compressStream2(cctx, ctypes.byref(ob), ctypes.byref(ib), 2 if b + 1 == blocks_per_frame else 1)   # ZSTD_e_end / ZSTD_e_flush
            assert not L.ZSTD_isError(r) and r == 0 and ib.pos == len(chunk)
            total += len(chunk)
        L.ZSTD_freeCCtx(cctx)
        frames.append(dst.raw[:ob.pos])
        caps.append(total)
    return frames, caps


def references(frames, caps):
    """The oracle's output of every frame; every input must decode (status 0), so that nothing is silently left out."""
    refs = []
    for i, (fr, cap) in enumerate(zip(frames, caps)):
        st, ref, _ = oracle.decode_frame(fr, cap=cap)
        assert st == 0, (i, st)
        refs.append(ref)
    return refs
