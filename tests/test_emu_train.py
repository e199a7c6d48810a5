"""Dictionary training (the cz_train_*_kernel launches of cz_dictionary_train_device, the unmodified kernel sources) on the CPU
SIMT emulator under ASan + UBSan (tests/emu/emu_train.cpp): what the selection picks and where it puts it, the dictionary's validity
read with a parser of the tests' own, with the oracle and with libzstd, the edges, the argument errors, determinism.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import dict_records as dr
import emu_train_runner as emu
import train_data as td

pytestmark = pytest.mark.xdist_group(name="emu_train")
INVALID_ARG = 901


@pytest.fixture(scope="module")
def users150():
    samples, cap = td.manifest_inputs()["users150"]
    return samples, cap, emu.train(samples, cap)


def test_planted_string_is_taken_whole_and_once():
    samples, s = td.planted()
    assert all(b.count(s) == 1 for b in samples)
    raw = emu.train(samples, 2048)
    content = td.check_valid(raw, 2048)["content"]
    assert content.count(s) == 1                                        # a second copy would mean the counters were not zeroed


def test_the_more_frequent_string_ends_later():
    samples, a, b = td.two_planted()
    assert sum(a in x for x in samples) == 58 and sum(b in x for x in samples) == 19
    content = td.check_valid(emu.train(samples, 2048), 2048)["content"]
    assert content.count(a) == 1 and content.count(b) == 1
    assert content.index(a) + len(a) > content.index(b) + len(b)       # chosen earlier: nearer the end, smaller offsets


def test_validity(users150):
    samples, cap, raw = users150
    d = td.check_valid(raw, cap)
    assert len(d["content"]) > cap // 2
    z = dr.libzstd()
    if z:
        held = [b for j, b in dr.records(20, seed=7) if j == 0]
        assert len(held) == 20
        for b in held:
            frame = dr.zstd_compress_dict(b, raw, 1)
            assert dr.zstd_decompress_dict(frame, len(b), raw) == b
            assert dr.zstd_decompress_dict(frame, len(b), None) != b     # the frame needs the dictionary
        lib = z[0]
        lib.ZDICT_getDictID.restype, lib.ZDICT_getDictID.argtypes = ctypes.c_uint, [ctypes.c_void_p, ctypes.c_size_t]
        assert lib.ZDICT_getDictID(raw, len(raw)) == d["id"]


def test_samples_shorter_than_the_capacity_are_the_content():
    samples = [b"", b"first sample, long enough", b"x", b"1234567", b"second sample: the content is all of them, in order"]
    raw = emu.train(samples, 1024)
    assert td.check_valid(raw, 1024)["content"] == b"".join(samples)


def test_short_samples_among_longer_ones():
    long = td.family_records(1, 40)
    samples = [b"", b"\xf8"] + long[:20] + [b"\xf9" * 7, b""] + long[20:] + [b"\xfa" * 7]
    raw = emu.train(samples, 1024)
    content = td.check_valid(raw, 1024)["content"]
    assert len(content) > 352                                           # more than half of the room was filled ...
    assert not set(content) & {0xF8, 0xF9, 0xFA}                        # ... and a sample without a d-mer gives no byte


def test_segment_len_16():
    raw = emu.train(td.family_records(2, 30), 1024, segment_len=16)
    assert len(td.check_valid(raw, 1024)["content"]) > 352


def test_segment_len_4096():
    recs = td.family_records(2, 24)
    a, b = b"".join(recs[:20])[:4300], b"".join(recs[20:])[:1000]
    assert len(a) == 4300 and len(b) == 1000
    raw = emu.train([b, a], 4096 + 320, segment_len=4096)               # room for one segment: one window of 4096 bytes of a
    content = td.check_valid(raw, 4096 + 320)["content"]
    assert len(content) == 4096 and content in a


def test_dict_id_given():
    samples, cap = td.manifest_inputs()["users150"]
    raw = emu.train(samples[:30], 1024, dict_id=0x12345678)
    assert td.check_valid(raw, 1024, dict_id=0x12345678)["id"] == 0x12345678
    assert emu.train(samples[:30], 1024, params=False)[8:] == raw[8:]   # NULL parameters: the defaults, here all but the ID


def test_argument_errors_write_nothing():
    ok = [b"a sample of more than eight bytes"] * 4
    cases = [
        dict(samples=ok, capacity=1023),
        dict(samples=[], capacity=2048),
        dict(samples=ok, capacity=2048, reserved=(0, 0, 0, 0, 0, 1)),
        dict(samples=ok, capacity=2048, reserved=(7, 0, 0, 0, 0, 0)),
        dict(samples=ok, capacity=2048, segment_len=15),
        dict(samples=ok, capacity=2048, segment_len=4097),
        dict(samples=ok, capacity=2048, claimed=[1 << 29] * 4),          # 2 GiB in all
        dict(samples=ok[:1], capacity=2048, claimed=[1 << 31]),
        dict(samples=[b"1234567", b"", b"abc"], capacity=2048),          # no sample of 8 bytes
    ]
    for kw in cases:
        status, _, n, region = emu.run(**kw)
        assert status == INVALID_ARG and n == 0, kw
        assert set(region) <= {0xEE}, kw


def test_determinism_and_sample_order(users150):
    samples, cap, raw = users150
    assert emu.train(samples, cap) == raw
    other = emu.train(list(reversed(samples)), cap)
    td.check_valid(other, cap)
