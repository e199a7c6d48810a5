"""Compression with dictionaries (cz_dict_setup_kernel -> cz_enc_dict_prep_kernel -> cz_compress_frames_dict_kernel, the
unmodified kernel sources) on the CPU SIMT emulator under ASan + UBSan (tests/emu/emu_encode_dict.cpp).  Every frame must decode
to its input under the oracle with its dictionary and under libzstd where the host has it.  No GPU needed."""
import os
import random

import pytest

import compress_frames as cf
import dict_frames as dfr
import dict_records as dr
import emu_encode_dict_runner as emu
import emu_encode_runner as emu0
import oracle

pytestmark = pytest.mark.xdist_group(name="emu_encode_dict")

GOLDEN_DICT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dict")
OUTPUT_TOO_SMALL, INVALID_ARG = 900, 901


def golden_dict(name):
    return open(os.path.join(GOLDEN_DICT, name), "rb").read()


def check(buffers, dict_of, got, checksum=False):
    """Every frame decodes to its input (oracle with its dictionary, and libzstd); nothing past bytes_written is touched.
    dict_of[i]: the raw dictionary of frame i, or None.  Returns the frames."""
    frames = []
    for i, (b, (r, region)) in enumerate(zip(buffers, got)):
        assert int(r["status"]) == 0, i
        n = int(r["bytes_written"])
        frame = region[:n]
        assert n <= emu.compress_bound(len(b)), (i, n)
        assert set(region[n:]) <= {0xEE}, f"{i}: bytes past bytes_written were touched"
        assert int(r["bytes_read"]) == len(b)
        if dict_of[i] is None:
            st, out, info = oracle.decode_frame(frame, cap=len(b) + 64)
            assert st == 0 and out == b and info["consumed"] == n, (i, st)
        else:
            st, out = oracle.decode_frame_with_dict(frame, oracle.Dictionary(dict_of[i]), cap=len(b) + 64)
            assert st == 0 and out == b, (i, st)
        if checksum:
            assert int(r["checksum"]) == oracle.xxh64(b) & 0xFFFFFFFF
        if dr.libzstd():
            assert dr.zstd_decompress_dict(frame, len(b), dict_of[i]) == b, f"{i}: libzstd"
        frames.append(frame)
    return frames


@pytest.fixture(scope="module")
def records():
    recs = dr.records(200)
    dicts = dr.dictionaries()
    got = emu.run([b for _, b in recs], dicts, index=[j for j, _ in recs])
    frames = check([b for _, b in recs], [dicts[j] for j, _ in recs], got)
    return recs, dicts, frames


def test_records_round_trip_and_dictionary_use(records):
    recs, dicts, frames = records
    kinds = [dfr.blocks(f) for f in frames]
    assert any(b[1] == "treeless" for k in kinds for b in k), "no frame used the dictionary's Huffman code"
    assert any(b[3] and 3 in b[3] for k in kinds for b in k), "no frame used a dictionary FSE table"
    # matches into the content: with the content changed (tables kept), some frames no longer decode to their input
    changed = 0
    for (j, b), f in zip(recs[:200], frames[:200]):
        raw = dicts[j]
        off = oracle.Dictionary(raw).info["content_off"]
        bent = raw[:off] + bytes(x ^ 0x5A for x in raw[off:])
        st, out = oracle.decode_frame_with_dict(f, oracle.Dictionary(bent), cap=len(b) + 64)
        changed += st != 0 or out != b
    assert changed > 50


def test_records_header_ids(records):
    recs, dicts, frames = records
    want = {0: 1, 1: 2, 2: 4, 3: 4}                                    # IDs 0xC5, 0x9C41, 0x123457, 0x9ABCDEF1
    for (j, _), f in zip(recs, frames):
        assert dfr.header_id(f) == (want[j], oracle.Dictionary(dicts[j]).info["id"])
    got = emu.run([b for _, b in recs[:8]], dicts, index=[j for j, _ in recs[:8]], flags=emu.NO_DICT_ID)
    nf = check([b for _, b in recs[:8]], [dicts[j] for j, _ in recs[:8]], got)
    assert all(dfr.header_id(f) == (0, 0) for f in nf)


def test_records_size_bar(records):
    recs, dicts, frames = records
    total = sum(len(f) for f in frames)
    plain = emu0.run([b for _, b in recs])
    plain_total = sum(int(r["bytes_written"]) for r, _ in plain)
    assert total <= 0.55 * plain_total, (total, plain_total)
    if dr.libzstd():
        ref = sum(len(dr.zstd_compress_dict(b, dicts[j], 1)) for j, b in recs)
        assert total <= 1.4 * ref, (total, ref)


def test_golden_dictionaries_and_special_inputs():
    sp = sorted(cf.special_inputs().items())
    d, dh = golden_dict("dict.bin"), golden_dict("dict_hist.bin")
    orig = [open(os.path.join(GOLDEN_DICT, n), "rb").read() for n in sorted(os.listdir(GOLDEN_DICT)) if n.endswith(".orig")]
    bufs = [b for _, b in sp] + orig + orig
    idx = [0] * (len(sp) + len(orig)) + [1] * len(orig)
    got = emu.run(bufs, [d, dh], index=idx, flags=emu.CHECKSUM)
    check(bufs, [(d, dh)[i] for i in idx], got, checksum=True)


def test_offset_history_starts_from_the_dictionary():
    dh = golden_dict("dict_hist.bin")
    h0 = oracle.Dictionary(dh).info["hist0"]
    assert h0 != 1
    rng = random.Random(5)
    x = bytes(rng.randrange(256) for _ in range(h0))
    bufs = [b"ab" + b"x" * 40, b"ab" + x * 6, b"q" + x * 3 + b"tail"]
    got = emu.run(bufs, [dh], index=None)
    frames = check(bufs, [dh] * 3, got)
    # decoded from the default history instead, the repeat-offset frame comes out wrong
    st, out, _ = oracle.decode_frame(frames[1], cap=len(bufs[1]) + 64)
    assert st != 0 or out != bufs[1]


def test_no_dict_frames_are_the_plain_frames():
    sp = sorted(cf.special_inputs().items())
    bufs = [b for _, b in sp] + [b for _, b in cf.corpus_originals(max_len=6000)[:12]]
    d = golden_dict("dict.bin")
    idx = [emu.NO_DICT if i % 3 else 0 for i in range(len(bufs))]
    got = emu.run(bufs, [d], index=idx, flags=emu.CHECKSUM)
    plain = emu0.run(bufs, flags=emu.CHECKSUM)
    for i, ((r, reg), (r0, reg0)) in enumerate(zip(got, plain)):
        if idx[i] == emu.NO_DICT:
            assert reg == reg0 and int(r["bytes_written"]) == int(r0["bytes_written"]), i
    check(bufs, [None if i == emu.NO_DICT else d for i in idx], got, checksum=True)


def test_bad_index_fails_the_frame_alone():
    d = golden_dict("dict.bin")
    bufs = [b"hello hello hello hello", b"abcdefgh" * 30, b"x" * 100]
    got = emu.run(bufs, [d], index=[0, 1, emu.NO_DICT])
    assert int(got[1][0]["status"]) == INVALID_ARG and int(got[1][0]["bytes_written"]) == 0 and set(got[1][1]) == {0xEE}
    check([bufs[0], bufs[2]], [d, None], [got[0], got[2]])
    got = emu.run(bufs[:1], [], index=[0])                              # no dictionaries at all
    assert int(got[0][0]["status"]) == INVALID_ARG and set(got[0][1]) == {0xEE}


def test_cross_block_table_state():
    """Large inputs: the dictionary's tables are used only while no Compressed block has replaced them; offsets stay in the window."""
    rng = random.Random(11)
    recs = dr.records(700, seed=3)
    users = b"".join(b for j, b in recs if j == 0)
    mixed = bytes(rng.randrange(256) for _ in range(30000)) + users
    big = (users * 20)[: 3 << 20]
    bufs = [users[: 200 << 10], mixed[: 200 << 10], big]
    assert len(big) == 3 << 20
    d = dr.dictionaries()[0]
    got = emu.run(bufs, [d], index=None)
    frames = check(bufs, [d] * 3, got)
    for f in frames:
        own_huf, predefined = False, set()
        for btype, lit, n, modes in dfr.blocks(f):
            if btype != "compressed":
                continue
            assert not (own_huf and lit == "treeless")
            if n:
                for field in range(3):
                    assert not (field in predefined and modes[field] == 3)
                    if modes[field] == 0:
                        predefined.add(field)
            own_huf |= lit == "huffman"
    assert not (frames[2][4] >> 5) & 1                                  # 3 MiB: not single-segment, a 1 MiB window
    assert dfr.header_id(frames[2]) == (1, 0xC5)


def test_bound_holds_with_a_4_byte_id_and_the_checksum():
    d = dr.dictionaries()[3]                                            # ID 0x9ABCDEF1: a 4-byte field
    rng = random.Random(3)
    data = bytes(rng.randrange(256) for _ in range(3 << 20))
    (r, region), = emu.run([data], [d], index=[0], flags=emu.CHECKSUM)
    frame = check([data], [d], [(r, region)], checksum=True)[0]
    assert dfr.header_id(frame)[0] == 4
    assert len(frame) == emu.compress_bound(len(data))                 # incompressible: exactly the bound


def test_small_output_caps():
    recs = dr.records(2)
    dicts = dr.dictionaries()
    bufs, idx = [b for _, b in recs], [j for j, _ in recs]
    ok = emu.run(bufs, dicts, index=idx)
    need = [int(r["bytes_written"]) for r, _ in ok]
    caps = [1, 5, need[2] - 1, need[3] - 4, need[4], 0, 12, need[7] - 1]
    got = emu.run(bufs, dicts, index=idx, caps=caps)
    for i, (r, region) in enumerate(got):
        w = int(r["bytes_written"])
        assert set(region[w:]) <= {0xEE}, i
        if caps[i] >= need[i]:
            assert int(r["status"]) == 0 and region[:w] == ok[i][1][:need[i]]
        else:
            assert int(r["status"]) == OUTPUT_TOO_SMALL, i
