"""Helpers of the dictionary compression tests: the Dictionary_ID field of a frame header and, per block, the literals type and
the sequence modes.  Test infrastructure only."""


def header_id(frame):
    """(width of the Dictionary_ID field, its value)."""
    fhd = frame[4]
    single, flag = (fhd >> 5) & 1, fhd & 3
    width = (0, 1, 2, 4)[flag]
    at = 5 + (0 if single else 1)
    return width, int.from_bytes(frame[at:at + width], "little")


def blocks(frame):
    """[(block type, literals type or None, number of sequences, (LL, OF, ML) modes or None)] — modes 0 Predefined ... 3 Repeat."""
    fhd = frame[4]
    fcs_flag, single, dict_flag = fhd >> 6, (fhd >> 5) & 1, fhd & 3
    pos = 5 + (0 if single else 1) + (0, 1, 2, 4)[dict_flag] + ((1 if single else 0), 2, 4, 8)[fcs_flag]
    out = []
    while True:
        bh = int.from_bytes(frame[pos:pos + 3], "little")
        last, btype, size = bh & 1, (bh >> 1) & 3, bh >> 3
        body = frame[pos + 3: pos + 3 + (1 if btype == 1 else size)]
        if btype != 2:
            out.append((("raw", "rle", "compressed", "reserved")[btype], None, 0, None))
        else:
            lt, sf = body[0] & 3, (body[0] >> 2) & 3
            if lt < 2:
                hdr = 1 if sf in (0, 2) else (2 if sf == 1 else 3)
                v = int.from_bytes(body[:hdr], "little")
                regen = v >> 3 if hdr == 1 else v >> 4
                at = hdr + (regen if lt == 0 else 1)
            else:
                hdr, bits = (3, 10) if sf < 2 else ((4, 14) if sf == 2 else (5, 18))
                v = int.from_bytes(body[:hdr], "little")
                at = hdr + ((v >> (4 + bits)) & ((1 << bits) - 1))
            b0 = body[at]
            if b0 < 128:
                n, at = b0, at + 1
            elif b0 < 255:
                n, at = ((b0 - 128) << 8) + body[at + 1], at + 2
            else:
                n, at = body[at + 1] + (body[at + 2] << 8) + 0x7F00, at + 3
            modes = None if n == 0 else (body[at] >> 6, (body[at] >> 4) & 3, (body[at] >> 2) & 3)
            out.append(("compressed", ("raw", "rle", "huffman", "treeless")[lt], n, modes))
        pos += 3 + len(body)
        if last:
            return out
