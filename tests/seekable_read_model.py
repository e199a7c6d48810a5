"""An independent model of reading byte ranges out of a seekable stream, in pure Python: the oracle of the
seekable-read tests.  From the table's entries, the ranges and out_align it gives the selection, the seven per-frame arrays, the
spans, the info record and the refusals of cz_seekable_locate_*; the final truth for a gather is `gathered`.  It works frame by
frame and range by range with sets and lists, nothing like the kernels or the host functions.  Test infrastructure only."""
import bisect

import seekable_model as fmt

OK, SEEK_TABLE, INVALID_ARG, TOO_SMALL = fmt.OK, fmt.SEEK_TABLE, fmt.INVALID_ARG, fmt.TOO_SMALL
MAX_RANGES = fmt.MAX_FRAMES
ARRAYS = ("frame", "in_off", "in_len", "out_off", "out_cap", "checksum", "content_off")


def info(status, ents, detail=0, selected=0, out_bytes=0, dst_bytes=0, reason=0):
    if ents is None:
        return dict(status=status, reason=reason, frames=0, content_bytes=0, selected=0, out_bytes=0, dst_bytes=0, detail=0, has_checksums=0, reserved=0)
    return dict(status=status, reason=reason, frames=len(ents), content_bytes=sum(d for _, d, _ in ents), selected=selected, out_bytes=out_bytes,
                dst_bytes=dst_bytes, detail=detail, has_checksums=int(bool(ents) and ents[0][2] is not None), reserved=0)


def locate_entries(ents, ranges, out_align=1, frames_cap=None, per_frame=True, has_checksums=None):
    """(info, arrays, spans) for a table with the entries `ents` [(Compressed_Size, Decompressed_Size, Checksum or None)]: `arrays`
    a dict of the seven per-frame lists and `spans` a list of (dst_off, src_off, sel_first, sel_count), both None on a refusal.
    frames_cap None: as many as are selected."""
    content = sum(d for _, d, _ in ents)
    base = info(OK, ents)
    if has_checksums is not None:
        base["has_checksums"] = has_checksums
    for j, (o, l) in enumerate(ranges):
        if o > content or o + l > content:
            return dict(base, status=INVALID_ARG, detail=j), None, None
    starts, at = [], 0
    for _, d, _ in ents:
        starts.append(at)
        at += d
    # frame i holds content bytes [starts[i], starts[i] + d): it is wanted when a non-empty range overlaps that interval
    wanted = set()
    touched = []
    for o, l in ranges:
        # (bisect only narrows the candidates: frames in front of lo end at or before o, frames from hi on start at or behind o + l)
        lo, hi = max(bisect.bisect_right(starts, o) - 1, 0), bisect.bisect_left(starts, o + l)
        mine = [i for i in range(lo, hi) if ents[i][1] and starts[i] < o + l and o < starts[i] + ents[i][1]] if l else []
        touched.append(mine)
        wanted.update(mine)
    sel = sorted(wanted)
    place = {f: s for s, f in enumerate(sel)}
    out_off, pos, need, comp_at = [], 0, 0, []
    at = 0
    for c, _, _ in ents:
        comp_at.append(at)
        at += c
    for f in sel:
        d = ents[f][1]
        out_off.append(pos)
        need = pos + d
        pos += -(-d // out_align) * out_align
    dst = sum(l for _, l in ranges)
    base.update(selected=len(sel), out_bytes=need, dst_bytes=dst)
    if per_frame and frames_cap is not None and len(sel) > frames_cap:
        return dict(base, status=TOO_SMALL), None, None
    arrays = dict(frame=sel, in_off=[comp_at[f] for f in sel], in_len=[ents[f][0] for f in sel], out_off=out_off,
                  out_cap=[ents[f][1] for f in sel], checksum=[ents[f][2] or 0 for f in sel], content_off=[starts[f] for f in sel])
    spans, at = [], 0
    for (o, l), mine in zip(ranges, touched):
        if mine:
            assert [place[f] for f in mine] == list(range(place[mine[0]], place[mine[0]] + len(mine)))   # consecutive in the selection
            spans.append((at, out_off[place[mine[0]]] + o - starts[mine[0]], place[mine[0]], len(mine)))
        else:
            spans.append((at, 0, 0, 0))
        at += l
    return base, arrays, spans


def locate(stream, ranges, out_align=1, frames_cap=None, per_frame=True):
    """The same for a stream: a damaged table is (info with SEEK_TABLE and the reason, None, None)."""
    reason, ents = fmt.parse(stream)
    if reason:
        return info(SEEK_TABLE, None, reason=reason), None, None
    return locate_entries(ents, ranges, out_align, frames_cap, per_frame, has_checksums=stream[-5] >> 7)


def decoded(contents, arrays, out_bytes, fill=0xEE):
    """What one decode of the selected frames leaves: each frame's content at its out_off, `fill` in the alignment gaps."""
    buf = bytearray([fill]) * out_bytes
    for f, o in zip(arrays["frame"], arrays["out_off"]):
        buf[o:o + len(contents[f])] = contents[f]
    return bytes(buf)


def gathered(contents, ranges):
    """The final truth of a gather: the ranges' bytes back to back."""
    content = b"".join(contents)
    return b"".join(content[o:o + l] for o, l in ranges)
