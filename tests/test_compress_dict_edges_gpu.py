"""cz_compress_batch_dict_device on the MI355X with the hand-built dictionaries and edge inputs of tests/dict_edges.py: the
device's frames equal the emulator's (sha256 manifest) for flags 0 and CZ_COMPRESS_CHECKSUM, the reversed batch at another input
shift, and the host path; the oracle and libzstd decode them with the dictionary and their predicates hold; this library's decoder
decodes them with cz_context_set_dictionaries in the single launch and in the pre-pass pipeline with checksums verified.  An edge
the emulator does not take (emu=False: content_leaves_window) is held to the oracle and its predicate only.  The order of the
dictionaries set for compression and a dictionary set in two slots do not change a frame.  Run with `pytest -m gpu`."""
import hashlib
import json
import os

import pytest

import compress_edges as ce
import dict_build as db
import dict_edges as de
import dict_records as dr
from test_compress_dict_gpu import POISON, device_compress, frames_of

pytestmark = pytest.mark.gpu
MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compress_dict_edges", "manifest.json")


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
    return de.edges()


@pytest.fixture(scope="module")
def batch(edges):
    return de.batch(edges)


@pytest.fixture(scope="module")
def compressed(cz, ctx, edges, batch):
    """{checksum: frames in edge order}; each batch is also compressed reversed, the dictionaries in reversed order too, at another
    input shift, and through the host path, and compared."""
    bufs, raws, idx = batch
    ds = [cz.Dictionary(ctx, raw) for raw in raws]
    out = {}
    for checksum in (False, True):
        ctx.set_compress_dictionaries(ds)
        got = device_compress(cz, ctx, bufs, idx, checksum=checksum)
        for e, (r, region) in zip(edges, got):
            n = int(r["bytes_written"])
            assert int(r["status"]) == 0 and int(r["bytes_read"]) == len(e.data), e.name
            assert n <= cz.compress_bound(len(e.data)) and set(region[n:]) <= {POISON}, e.name
        frames = frames_of(got)
        assert [f for _, f in cz.compress_batch_host_dict(bufs, idx, ctx, checksum=checksum)] == frames
        ctx.set_compress_dictionaries(ds[::-1])
        rev = device_compress(cz, ctx, bufs[::-1], [len(ds) - 1 - i for i in idx[::-1]], checksum=checksum, in_shift=1)
        assert frames_of(rev)[::-1] == frames
        out[checksum] = frames
    ctx.set_compress_dictionaries([])
    return out


def test_frames_equal_the_emulators(edges, compressed):
    m = json.load(open(MANIFEST))
    emu = [e for e in edges if e.emu]
    assert m["names"] == [e.name for e in emu]
    for checksum, flags in ((False, "0"), (True, "1")):
        got = [hashlib.sha256(fr).hexdigest() for e, fr in zip(edges, compressed[checksum]) if e.emu]
        bad = [e.name for e, g, w in zip(emu, got, m["flags"][flags]) if g != w]
        assert not bad, (flags, bad)


def test_decoders_and_predicates(edges, compressed):
    import oracle
    for checksum in (False, True):
        for e, fr in zip(edges, compressed[checksum]):
            st, out = oracle.decode_frame_with_dict(fr, oracle.Dictionary(e.dictionary), cap=len(e.data) + 64)
            assert st == 0 and out == e.data, (e.name, checksum, st)
            if checksum:
                assert int.from_bytes(fr[-4:], "little") == oracle.xxh64(e.data) & 0xFFFFFFFF, e.name
            if dr.libzstd():
                got = dr.zstd_decompress_dict(fr, len(e.data), e.dictionary)
                if e.dname in db.LIBZSTD_REFUSES:
                    assert got is None, e.name
                else:
                    assert got == e.data, e.name
            a = ce.analyse(fr, e.data, dictionary=e.dictionary)
            e.check(a)
            de.check_header(e, fr)
            assert all(o <= ce.WINDOW for b in a["blocks"] if b["type"] == "compressed" for o in b["offsets"]), e.name


@pytest.mark.parametrize("prepass", [False, True], ids=["single_launch", "prepass_verify"])
def test_library_decoder(cz, edges, batch, compressed, prepass):
    """The frames name their dictionaries by ID; the one without an ID (id_0) goes to the no_id dictionary."""
    _, raws, idx = batch
    for checksum in (False, True):
        dctx = cz.Context(0)
        try:
            ds = [cz.Dictionary(dctx, raw) for raw in raws]
            no_id = [d for d in ds if d.id == 0]
            assert len(no_id) == 1
            dctx.set_dictionaries([d for d in ds if d.id != 0], no_id=no_id[0])
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


def test_slot_order_and_shared_slots(cz, ctx, edges, compressed):
    """[A, B], then [B, A] with the indices swapped, then [A, B] again: the same frames.  One Dictionary object in two slots: the
    frames of slot 1 equal those of slot 0."""
    pick = [e for e in edges if e.dname in ("bnd_5", "rep_21")]
    assert [e.dname for e in pick] == ["bnd_5", "rep_21"]
    want = [compressed[False][edges.index(e)] for e in pick]
    bufs = [e.data for e in pick]
    a, b = (cz.Dictionary(ctx, e.dictionary) for e in pick)
    try:
        for order, idx in (([a, b], [0, 1]), ([b, a], [1, 0]), ([a, b], [0, 1])):
            ctx.set_compress_dictionaries(order)
            assert frames_of(device_compress(cz, ctx, bufs, idx)) == want, idx
        ctx.set_compress_dictionaries([a, a])
        assert frames_of(device_compress(cz, ctx, [bufs[0], bufs[0]], [0, 1])) == [want[0], want[0]]
    finally:
        ctx.set_compress_dictionaries([])
