"""cz_compress_batch_device on the MI355X at the edges of the zstd format (tests/compress_edges.py): the device's frames equal the
emulator's (sha256 manifest) for flags 0 and CZ_COMPRESS_CHECKSUM, whichever workgroup takes which frame; the oracle decodes them and
their predicates hold; this library's decoder decodes them byte for byte in the single launch and in the pre-pass pipeline with
checksums verified.  The first GPU run of blocks of 32 512+ sequences and of matches exactly 1 MiB back through the decoder's
kernels.  The one input too large for the emulator (big_window_exact, 2.1 MiB) has no manifest entry: it is checked against the
oracle and its predicate only.  Run with `pytest -m gpu`."""
import hashlib
import json
import os

import pytest

import compress_edges as ce
import compress_frames as cf
from test_compress_gpu import POISON, device_compress, frames_of

pytestmark = pytest.mark.gpu
MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compress_edges", "manifest.json")


@pytest.fixture(scope="module")
def cz():
    import torch  # noqa: F401
    import cairo_zstd_amd as m
    assert os.path.exists(m._lib.LIB_PATH), "libcairo_zstd_amd.so missing: run __graft_entry__.build()"
    return m


@pytest.fixture(scope="module")
def ctx(cz):
    c = cz.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def edges():
    return ce.edges()


@pytest.fixture(scope="module")
def compressed(cz, ctx, edges):
    """{checksum: frames in edge order}, each batch also compressed reversed (at another input shift) and compared."""
    out = {}
    for checksum in (False, True):
        got, _, _, _ = device_compress(cz, ctx, [e.data for e in edges], checksum=checksum)
        for e, (r, region) in zip(edges, got):
            n = int(r["bytes_written"])
            assert int(r["status"]) == 0 and int(r["bytes_read"]) == len(e.data), e.name
            assert n <= cz.compress_bound(len(e.data)) and set(region[n:]) <= {POISON}, e.name
        frames = frames_of(got)
        rev, _, _, _ = device_compress(cz, ctx, [e.data for e in edges][::-1], in_shift=1, checksum=checksum)
        assert frames_of(rev)[::-1] == frames
        out[checksum] = frames
    return out


def test_frames_equal_the_emulators(edges, compressed):
    m = json.load(open(MANIFEST))
    emu = [e for e in edges if e.emu]
    assert m["names"] == [e.name for e in emu]
    for checksum, flags in ((False, "0"), (True, "1")):
        got = [hashlib.sha256(fr).hexdigest() for e, fr in zip(edges, compressed[checksum]) if e.emu]
        bad = [e.name for e, g, w in zip(emu, got, m["flags"][flags]) if g != w]
        assert not bad, (flags, bad)


def test_oracle_decodes_and_predicates_hold(edges, compressed):
    import oracle
    for checksum in (False, True):
        for e, fr in zip(edges, compressed[checksum]):
            st, out, info = oracle.decode_frame(fr, cap=len(e.data) + 64)
            assert st == 0 and out == e.data and info["consumed"] == len(fr), (e.name, checksum, st)
            if checksum:
                assert info["has_checksum"] and info["checksum"] == oracle.xxh64(e.data) & 0xFFFFFFFF, e.name
            if cf.libzstd():
                assert cf.libzstd_decompress(fr, len(e.data)) == e.data, e.name
            e.check(ce.analyse(fr, e.data))


@pytest.mark.parametrize("prepass", [False, True], ids=["single_launch", "prepass_verify"])
def test_library_decoder(cz, edges, compressed, prepass):
    for checksum in (False, True):
        dctx = cz.Context(0)
        try:
            if prepass:
                dctx.set_chain_arena(64 << 20, min_sequences=0)
                dctx.set_literal_arena(32 << 20)
                dctx.set_verify_checksum(True)
            dec = cz.decode_batch_host(compressed[checksum], [len(e.data) + 64 for e in edges], dctx)
        finally:
            dctx.close()
        for e, (r, out) in zip(edges, dec):
            assert int(r["status"]) == 0 and out == e.data, (e.name, checksum, prepass, int(r["status"]))
            if prepass and checksum:
                assert r["flags"] & cz.RESULT_CHECKSUM_MATCH, e.name
