"""The batched compressor (cz_compress_frames_kernel, czstd_enc.hip unmodified) on the CPU SIMT emulator under ASan + UBSan
(tests/emu/emu_encode.cpp).  Every frame must decode to its input under the oracle (status 0, every byte consumed), stay within
cz_compress_bound, and decode under libzstd where the host has it.  No GPU needed."""
import pytest

import compress_frames as cf
import emu_encode_runner as emu
import oracle

pytestmark = pytest.mark.xdist_group(name="emu_encode")


def check(buffers, got, flags=0):
    z = cf.libzstd()
    for name, b, (r, region) in zip([n for n, _ in buffers], [b for _, b in buffers], got):
        assert int(r["status"]) == 0, name
        n = int(r["bytes_written"])
        frame = region[:n]
        assert n <= emu.compress_bound(len(b)), (name, n)
        assert set(region[n:]) <= {0xEE}, f"{name}: bytes past bytes_written were touched"
        assert int(r["bytes_read"]) == len(b)
        st, out, info = oracle.decode_frame(frame, cap=len(b) + 64)
        assert st == 0 and out == b and info["consumed"] == n, (name, st)
        assert info["content_size"] == len(b)
        if flags & emu.CHECKSUM:
            assert info["has_checksum"] and info["checksum"] == oracle.xxh64(b) & 0xFFFFFFFF, name
            assert int(r["checksum"]) == oracle.xxh64(b) & 0xFFFFFFFF
        if z:
            assert cf.libzstd_decompress(frame, len(b)) == b, f"{name}: libzstd"
    return {name: region[:int(r["bytes_written"])] for (name, _), (r, region) in zip(buffers, got)}


def test_emu_small_corpus_originals():
    bufs = cf.corpus_originals(max_len=6000)
    assert len(bufs) >= 40
    check(bufs, emu.run([b for _, b in bufs]))


def test_emu_format_edges():
    sp = cf.special_inputs()
    bufs = sorted(sp.items())
    frames = check(bufs, emu.run([b for _, b in bufs]))
    assert frames["empty"][-3:] == b"\x01\x00\x00"                      # one empty last Raw block
    assert cf.walk(frames["rle64k"]) == [("rle", {})]
    assert all(t == "raw" for t, _ in cf.walk(frames["random64k"]))
    assert cf.walk(frames["text_ascii"])[0][1]["desc"] == "direct"
    assert cf.walk(frames["all_bytes"])[0][1]["desc"] == "fse"
    assert cf.walk(frames["lit_under_1k"])[0][1] == {"lit": "huffman", "streams": 1, "desc": "direct"}
    assert cf.walk(frames["lit_over_1k"])[0][1] == {"lit": "huffman", "streams": 4, "desc": "direct"}
    assert cf.walk(frames["long_match"])[0][0] == "compressed" and len(frames["long_match"]) < 40   # one match of ML > 65 536


def test_emu_checksum():
    sp = cf.special_inputs()
    bufs = [("text_ascii", sp["text_ascii"]), ("three", sp["three"]), ("empty", b"")] + cf.corpus_originals(max_len=3000)[:6]
    check(bufs, emu.run([b for _, b in bufs], flags=emu.CHECKSUM), flags=emu.CHECKSUM)


def test_emu_output_too_small_leaves_the_rest():
    a, b = cf.special_inputs()["text_ascii"], cf.corpus_originals(max_len=6000)[-1][1]
    ok = emu.run([a, b])
    need = int(ok[0][0]["bytes_written"])
    got = emu.run([a, b], caps=[need - 1, emu.compress_bound(len(b))])
    assert int(got[0][0]["status"]) == 900                              # CZ_E_OUTPUT_TOO_SMALL
    w = int(got[0][0]["bytes_written"])
    assert w < need - 1 and set(got[0][1][w:]) == {0xEE}
    assert got[1] [1] == ok[1][1] and int(got[1][0]["status"]) == 0     # the neighbour as before
