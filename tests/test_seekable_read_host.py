"""Byte ranges out of a seekable stream on the CPU (cz_seekable_locate_host, cz_seekable_gather_host;
csrc/czstd_seekable_read_host.h) against the independent model in seekable_read_model.py, on streams built by seekable_model.build:
the selection, the seven per-frame arrays, the spans, the info record and the refusals through cairo_zstd_amd.locate_seekable and
the C ABI, the gathered bytes against slices of the content.  The same cases then go through the header alone in a stand-alone
program under ASan + UBSan (tests/emu/seekable_read_host_main.cpp), from exact-size heap blocks; no Python code runs under a
sanitizer.  No GPU needed.  Every test here fails without the feature: the entry points do not exist."""
import numpy as np
import pytest

import cairo_zstd_amd as cz
import seekable_model as fmt
import seekable_read_model as model
import seekable_read_runner as sr
from test_emu_seekable_read import (check_call, check_gathered, cycling, damaged_cases, gather_cases, locate_cases, some_ranges, table)


def test_the_symbols_and_the_records_exist():
    """Fails without the feature."""
    L = cz.lib()
    for name in ("cz_seekable_index_create_device", "cz_seekable_index_destroy", "cz_seekable_locate_device", "cz_seekable_gather_device",
                 "cz_seekable_locate_host", "cz_seekable_gather_host"):
        assert hasattr(L, name), name
    assert cz.SEEKABLE_READ_INFO_DTYPE == sr.READ_INFO_DTYPE and cz.SEEKABLE_READ_INFO_DTYPE.itemsize == 64
    assert cz.SEEKABLE_SPAN_DTYPE == sr.SPAN_DTYPE and cz.SEEKABLE_SPAN_DTYPE.itemsize == 24
    for name in ("SeekableIndex", "locate_seekable", "read_seekable"):
        assert name in cz.__all__ and hasattr(cz, name), name
    assert hasattr(cz.Context, "seekable_index") and hasattr(cz.Context, "seekable_gather_device")


def against_the_model(stream, ranges, align):
    info, *arrays, spans = cz.locate_seekable(stream, ranges, align)
    winfo, warrays, wspans = model.locate(stream, ranges, align)
    assert {k: int(info[k]) for k in winfo} == winfo
    if winfo["status"] == 0:
        assert [a.tolist() for a in arrays] == [warrays[k] for k in model.ARRAYS]
        assert [tuple(int(x) for x in sp) for sp in spans] == wspans
    else:
        assert all(a.size == 0 for a in arrays) and spans.size == 0
    return info, arrays, spans


@pytest.mark.parametrize("align", (1, 16, 256, 4096))
@pytest.mark.parametrize("n", (0, 1, 2, 17, 300, 4097))
def test_locate_seekable_is_the_models(n, align):
    sizes = cycling(n)
    stream = table(sizes, cks=bool(n & 1))
    for m in (0, 1, 65, 300):
        against_the_model(stream, some_ranges(sizes, m, 5 * n + m), align)
    info, arrays, _ = against_the_model(stream, [(0, sum(sizes))], align)
    assert arrays[0].tolist() == [i for i, s in enumerate(sizes) if s]


def test_locate_seekable_refuses_as_the_model_does():
    sizes = cycling(300)
    stream, content = table(sizes, cks=True), sum(sizes)
    good = some_ranges(sizes, 9, 7)
    for bad, at in (((content - 3, 4), 0), ((content - 3, 4), 5), ((content + 1, 0), 9), (((1 << 64) - 1, 2), 3), ((3, (1 << 64) - 1), 8)):
        info, _, _ = against_the_model(stream, good[:at] + [bad] + good[at:], 16)
        assert (int(info["status"]), int(info["detail"])) == (model.INVALID_ARG, at)
    for reason, c in damaged_cases():
        info, _, _ = against_the_model(c.stream, good, 1)
        assert (int(info["status"]), int(info["reason"])) == (model.SEEK_TABLE, reason)
    for align in (0, 3, 8192):
        assert int(cz.locate_seekable(stream, good, align)[0]["status"]) == model.INVALID_ARG, align


def test_host_argument_refusals_and_frames_cap():
    sizes = cycling(300)
    stream = np.frombuffer(table(sizes), dtype=np.uint8)
    good = np.array(some_ranges(sizes, 9, 7), dtype=np.uint64)
    off, ln = np.ascontiguousarray(good[:, 0]), np.ascontiguousarray(good[:, 1])
    info = np.zeros(1, dtype=cz.SEEKABLE_READ_INFO_DTYPE)
    L, none8 = cz.lib(), [None] * 8

    def locate(*a):
        return L.cz_seekable_locate_host(stream.ctypes.data, stream.size, *a)

    assert locate(off.ctypes.data, ln.ctypes.data, 9, 1, 0, *none8, None) == model.INVALID_ARG
    assert locate(None, ln.ctypes.data, 9, 1, 0, *none8, info.ctypes.data) == model.INVALID_ARG == int(info[0]["status"])
    assert locate(off.ctypes.data, None, 9, 1, 0, *none8, info.ctypes.data) == model.INVALID_ARG
    assert locate(off.ctypes.data, ln.ctypes.data, model.MAX_RANGES + 1, 1, 0, *none8, info.ctypes.data) == model.INVALID_ARG
    assert locate(None, None, 0, 1, 0, *none8, info.ctypes.data) == 0 and int(info[0]["selected"]) == 0
    assert locate(off.ctypes.data, ln.ctypes.data, 9, 1, 0, *none8, info.ctypes.data) == 0       # the sizing call needs no frames_cap
    k = int(info[0]["selected"])
    assert k == model.locate(stream.tobytes(), [tuple(r) for r in good.tolist()])[0]["selected"] > 1
    frame = np.full(k, 0xA5A5A5A5, dtype=np.uint32)
    assert locate(off.ctypes.data, ln.ctypes.data, 9, 1, k - 1, frame.ctypes.data, *[None] * 7, info.ctypes.data) == model.TOO_SMALL
    assert int(info[0]["selected"]) == k and (frame == 0xA5A5A5A5).all()
    assert locate(off.ctypes.data, ln.ctypes.data, 9, 1, k, frame.ctypes.data, *[None] * 7, info.ctypes.data) == 0
    assert frame.tolist() == model.locate(stream.tobytes(), [tuple(r) for r in good.tolist()])[1]["frame"]


@pytest.mark.parametrize("name", ("cyclic_0", "cyclic_7", "three_tiles_and_a_byte", "empty_ranges", "only_empty_ranges", "no_ranges",
                                  "across_frames_with_gaps"))
def test_gather_host_gives_the_slices_of_the_content(name):
    c = gather_cases()[name]
    m = len(c.ranges)
    r = np.array(c.ranges, dtype=np.uint64).reshape(m, 2)
    off, ln = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
    out_off, content_off = (np.array(c.arrays[k], dtype=np.uint64) for k in ("out_off", "content_off"))
    dec = np.frombuffer(c.decoded + b"\0", dtype=np.uint8)
    dst = np.full(len(c.want) + 32, 0xEE, dtype=np.uint8)
    spans = c.spans.copy()
    st = cz.lib().cz_seekable_gather_host(dec.ctypes.data, out_off.ctypes.data, content_off.ctypes.data, len(out_off), off.ctypes.data, ln.ctypes.data,
                                          spans.ctypes.data, m, dst.ctypes.data + 16, len(c.want))
    assert st == 0
    assert dst[16:16 + len(c.want)].tobytes() == c.want and (dst[:16] == 0xEE).all() and (dst[16 + len(c.want):] == 0xEE).all()
    if len(c.want):                                                     # a destination one byte short is refused, not overrun
        assert cz.lib().cz_seekable_gather_host(dec.ctypes.data, out_off.ctypes.data, content_off.ctypes.data, len(out_off), off.ctypes.data,
                                                ln.ctypes.data, spans.ctypes.data, m, dst.ctypes.data + 16, len(c.want) - 1) == model.INVALID_ARG
        assert cz.lib().cz_seekable_gather_host(None, out_off.ctypes.data, content_off.ctypes.data, len(out_off), off.ctypes.data,
                                                ln.ctypes.data, spans.ctypes.data, m, dst.ctypes.data + 16, len(c.want)) == model.INVALID_ARG


def test_the_header_alone_under_asan_and_ubsan():
    """czstd_seekable_read_host.h compiled by g++ with -fsanitize=address,undefined into a program of its own: the same answers, from
    exact-size heap blocks."""
    lc, gc, dc = locate_cases(), gather_cases(), damaged_cases()
    res = sr.run(sr.HOST, [c.blob for c in lc.values()] + [c.blob for c in gc.values()] + [c.blob for _, c in dc])
    for (name, c), (ret, tab, calls) in zip(lc.items(), res):
        assert ret == 0 and all(int(tab[k]) == v for k, v in c.inf.items()) and len(calls) == len(c.calls), name
        for q, (call, got) in enumerate(zip(c.calls, calls)):
            check_call(name, q, call, *got)
    for (name, c), (ret, block) in zip(gc.items(), res[len(lc):]):
        assert ret == 0, name
        check_gathered(name, c, block)
    for (reason, c), (ret, tab, calls) in zip(dc, res[len(lc) + len(gc):]):
        assert ret == fmt.SEEK_TABLE and int(tab["reason"]) == reason
