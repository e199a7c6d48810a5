"""An independent model of the seekable stream format, with `struct` only: the oracle of the seekable tests.

    frame 0 | ... | frame n-1 | 0x184D2A5E | Frame_Size = n * E + 9 | n x { Compressed_Size, Decompressed_Size, [Checksum] } |
    Number_Of_Frames | Seek_Table_Descriptor (1 byte: bit 7 Checksum_Flag, bits 6..2 reserved, bits 1..0 unused) | 0x8F92EAB1

Every field but the descriptor is 32 bits, little-endian; nothing is aligned.  E is 8 without checksums, 12 with them.
Test infrastructure only."""
import struct

SKIPPABLE_MAGIC, SEEKABLE_MAGIC, MAX_FRAMES = 0x184D2A5E, 0x8F92EAB1, 0x8000000
OK, SEEK_TABLE, INVALID_ARG, TOO_SMALL = 0, 909, 901, 900
REASONS = (1, 2, 3, 4, 5, 6)


def table(lengths, sizes, checksums=None, descriptor=None):
    """The skippable frame that follows the frames."""
    n = len(lengths)
    assert len(sizes) == n and (checksums is None or len(checksums) == n)
    e = 8 if checksums is None else 12
    out = [struct.pack("<II", SKIPPABLE_MAGIC, n * e + 9)]
    for i in range(n):
        out.append(struct.pack("<II", lengths[i], sizes[i]))
        if checksums is not None:
            out.append(struct.pack("<I", checksums[i]))
    if descriptor is None:
        descriptor = 0x80 if checksums is not None else 0
    out.append(struct.pack("<IBI", n, descriptor, SEEKABLE_MAGIC))
    return b"".join(out)


def build(frames, sizes, checksums=None):
    """The stream of `frames` (their decompressed sizes in `sizes`, optionally their checksums)."""
    return b"".join(bytes(f) for f in frames) + table([len(f) for f in frames], sizes, checksums)


def bound(frame_bytes, n, checksums=False):
    return frame_bytes + 8 + n * (12 if checksums else 8) + 9


def parse(stream):
    """(reason, entries): reason 0 and the entries [(Compressed_Size, Decompressed_Size, Checksum or None)], or the first of the six
    checks that fails and None."""
    ln = len(stream)
    if ln < 17:
        return 1, None
    n, desc, magic = struct.unpack_from("<IBI", stream, ln - 9)
    if magic != SEEKABLE_MAGIC:
        return 2, None
    if desc & 0x7C:
        return 3, None
    e = 12 if desc & 0x80 else 8
    if n > MAX_FRAMES or 17 + n * e > ln:
        return 4, None
    at = ln - 17 - n * e
    if struct.unpack_from("<II", stream, at) != (SKIPPABLE_MAGIC, n * e + 9):
        return 5, None
    ents = []
    for i in range(n):
        c, d = struct.unpack_from("<II", stream, at + 8 + i * e)
        ents.append((c, d, struct.unpack_from("<I", stream, at + 16 + i * e)[0] if e == 12 else None))
    if sum(c for c, _, _ in ents) != at:
        return 6, None
    return 0, ents


def info_of(stream):
    """What cz_seekable_info says of `stream` after an open of an empty range: a dict (detail left out)."""
    reason, ents = parse(stream)
    if reason:
        return dict(status=SEEK_TABLE, reason=reason, frames=0, frames_bytes=0, content_bytes=0, stream_bytes=0, has_checksums=0)
    return dict(status=OK, reason=0, frames=len(ents), frames_bytes=sum(c for c, _, _ in ents), content_bytes=sum(d for _, d, _ in ents),
                stream_bytes=len(stream), has_checksums=stream[-5] >> 7)


def open_range(stream, first=0, count=None, out_align=1):
    """(status, in_off, in_len, out_off, out_cap, checksums, need) of frames [first, first + count) of a well-formed stream."""
    reason, ents = parse(stream)
    assert reason == 0
    n = len(ents)
    if first > n or (count is not None and first + count > n):
        return INVALID_ARG, [], [], [], [], [], 0
    count = n - first if count is None else count
    at = sum(c for c, _, _ in ents[:first])
    in_off, in_len, out_off, out_cap, sums, out, need = [], [], [], [], [], 0, 0
    for c, d, s in ents[first:first + count]:
        in_off.append(at); in_len.append(c); out_off.append(out); out_cap.append(d); sums.append(s or 0)
        need = out + d
        at += c
        out += -(-d // out_align) * out_align
    return OK, in_off, in_len, out_off, out_cap, sums, need


def damaged(stream):
    """reason -> a stream with that defect, made from a well-formed `stream` with at least one frame whose table it damages."""
    reason, ents = parse(stream)
    assert reason == 0 and ents
    ln, e = len(stream), 12 if stream[-5] & 0x80 else 8
    at = ln - 17 - len(ents) * e
    b = bytearray(stream)

    def put(pos, fmt, *v):
        c = bytearray(b)
        struct.pack_into(fmt, c, pos, *v)
        return bytes(c)

    out = {
        1: bytes(b[-16:]),
        2: put(ln - 4, "<I", SEEKABLE_MAGIC ^ 0x100),
        3: put(ln - 5, "<B", b[ln - 5] | 0x10),
        4: put(ln - 9, "<I", len(stream)),                               # a table longer than the stream
        5: put(at + 4, "<I", len(ents) * e + 8),                         # Frame_Size wrong
        6: put(at + 8, "<I", ents[0][0] + 1),                            # the sizes no longer add up to the table's offset
    }
    for r, s in out.items():
        assert parse(s)[0] == r, (r, parse(s)[0])
    return out


def damaged_more(stream):
    """Further defects for the reasons that name two checks: [(reason, stream)]."""
    reason, ents = parse(stream)
    assert reason == 0 and ents
    ln, e = len(stream), 12 if stream[-5] & 0x80 else 8
    at = ln - 17 - len(ents) * e
    c4, c5 = bytearray(stream), bytearray(stream)
    struct.pack_into("<I", c4, ln - 9, MAX_FRAMES + 1)
    struct.pack_into("<I", c5, at, SKIPPABLE_MAGIC ^ 1)
    out = [(4, bytes(c4)), (5, bytes(c5))]
    for r, s in out:
        assert parse(s)[0] == r
    return out
