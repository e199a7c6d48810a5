"""Helpers of the CZ_COMPRESS_SPLIT tests (emulator and GPU): the blocks of a frame with their offsets, the offset code of a block's
first sequence, corpus text of any length.  Test infrastructure only."""
import compress_frames as cf


def blocks_of(frame):
    """(header length, [(offset of the block header, last, type, Block_Size, bytes of header + body)])."""
    fhd = frame[4]
    fcs_flag, single, dict_flag = fhd >> 6, (fhd >> 5) & 1, fhd & 3
    pos = hl = 5 + (0 if single else 1) + (0, 1, 2, 4)[dict_flag] + ((1 if single else 0), 2, 4, 8)[fcs_flag]
    out = []
    while True:
        bh = int.from_bytes(frame[pos:pos + 3], "little")
        last, btype, size = bh & 1, (bh >> 1) & 3, bh >> 3
        n = 3 + (1 if btype == 1 else size)
        out.append((pos, last, btype, size, n))
        pos += n
        if last:
            return hl, out


def of_default_symbols():
    """The symbol of every state of the Predefined Offset table (RFC 8878 §3.1.1.3.2.2.3 and §4.1.1: accuracy log 5)."""
    norm = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
    size, sym = 32, [0] * 32
    high = size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    return sym


def first_offset_code(block):
    """Offset code of the FIRST sequence of a Compressed block (header included) whose sequences use the Predefined tables: the
    stream is read from its end — closing bit, then the initial LL (6 bits), OF (5) and ML (6) states."""
    body = block[3:]
    lt, sf = body[0] & 3, (body[0] >> 2) & 3
    if lt < 2:                                                          # Raw / RLE literals
        hdr = (1, 2, 1, 3)[sf]
        regen = body[0] >> 3 if hdr == 1 else (int.from_bytes(body[:hdr], "little") >> 4)
        lsz = hdr + (regen if lt == 0 else 1)
    else:
        hdr = 3 if sf < 2 else (4 if sf == 2 else 5)
        bits = (10, 10, 14, 18)[sf]
        lsz = hdr + ((int.from_bytes(body[:hdr], "little") >> (4 + bits)) & ((1 << bits) - 1))
    seq = body[lsz:]
    n = seq[0]
    h = 1 if n < 128 else (2 if n < 255 else 3)
    assert n > 0 and seq[h] == 0, "sequences with the Predefined tables expected"
    v = int.from_bytes(seq[h + 1:], "little")
    top = v.bit_length() - 1                                            # the closing 1 bit
    of_state = (v >> (top - 11)) & 31
    return of_default_symbols()[of_state]


def text(n, skip=0):
    pool = b"".join(b for _, b in cf.corpus_originals())
    return (pool * ((n + skip) // len(pool) + 2))[skip:skip + n]
