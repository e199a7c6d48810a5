"""Every compress level through ONE context, then again on larger batches: the levels share cz_enc_launch in czstd_host.hip, each
with a scratch of its own that grows with the grid, so a level handed another level's scratch or stride, or a slot count that is
stale after growth, shows here as a frame that differs from what a fresh context writes for the same batch (and, most likely, as
a frame that does not decode).  Levels: plain, dict, split, fse, split+fse, fast, records, records+dict.

Passes: n = 1, then n = 3 (the grid of plain, dict, fse and fast is min(device, n): their scratch grows from one slot to three; the
split levels take the whole device at once, their plan array grows with n).  The records levels put a record on every WAVE, four to
a workgroup, so n = 3 is still one workgroup; a third pass with n = 9 (three workgroups) makes their scratch grow too, and runs
for every level.  Buffers are about 40 KiB of text; the first buffer of the split batches is two segments and a bit, so the segment
kernel has several units; the records levels take at most compress_record_max() = 32 KiB, so their buffers are the same text cut
to 24 KiB.  Run with `pytest -m gpu`."""
import random

import pytest

import dict_records as dr
from test_compress_dict_gpu import cz  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
PASSES = (1, 3, 9)
LEVELS = {"plain": {}, "dict": {}, "split": dict(split=True), "fse": dict(fse_tables=True), "split_fse": dict(split=True, fse_tables=True),
          "fast": dict(fast=True), "records": dict(records=True), "records_dict": dict(records=True)}


def text(seed, n=40 << 10):
    """compressible text-like bytes, as compress_frames.special_inputs makes its text"""
    rng = random.Random(seed)
    words = [bytes(rng.choice(b"etaoinshrdlucmfwyp") for _ in range(rng.randint(2, 9))) for _ in range(300)]
    return b" ".join(rng.choice(words) for _ in range(n // 5))[:n]


@pytest.fixture(scope="module")
def batches(cz):
    """(level, n) -> the buffers, made once"""
    texts = [text(100 + i) + bytes([i]) * i for i in range(max(PASSES))]        # (lengths differ a little)
    seg = cz.compress_split_segment()
    long = (texts[0] * (2 * seg // len(texts[0]) + 2))[:2 * seg + 1234]
    assert cz.compress_record_max() == 32 << 10
    out = {}
    for level in LEVELS:
        for n in PASSES:
            bufs = list(texts[:n])
            if level.startswith("split"):
                bufs[0] = long
            if level.startswith("records"):
                bufs = [b[:(24 << 10) + i] for i, b in enumerate(bufs)]
            out[level, n] = bufs
    return out


def compress(cz, ctx, level, bufs):
    if level.endswith("dict"):
        return cz.compress_batch_host_dict(bufs, None, ctx, **LEVELS[level])   # (no index: every buffer uses the one dictionary)
    return cz.compress_batch_host(bufs, ctx, **LEVELS[level])


def with_dictionary(cz, ctx):
    d = cz.Dictionary(ctx, dr.dictionaries()[0])
    ctx.set_compress_dictionaries([d])
    return d


def test_every_level_in_one_context_across_growth(cz, batches):
    shared = cz.Context(0)
    try:
        d = with_dictionary(cz, shared)
        got = {}
        for n in PASSES:                                                # every level at n, then every level at the next n
            for level in LEVELS:
                got[level, n] = compress(cz, shared, level, batches[level, n])
        for (level, n), res in got.items():
            bufs = batches[level, n]
            for i, (r, frame) in enumerate(res):
                assert int(r["status"]) == 0 and int(r["bytes_read"]) == len(bufs[i]) and len(frame) == int(r["bytes_written"]) > 0, (level, n, i, r)
            # back through the library's decoder
            try:
                if level.endswith("dict"):
                    shared.set_dictionaries([d], no_id=d)
                dec = cz.decode_batch_host([f for _, f in res], [len(b) + 64 for b in bufs], shared)
            finally:
                shared.set_dictionaries([])
            for i, ((r, out), b) in enumerate(zip(dec, bufs)):
                assert int(r["status"]) == 0 and out == b, (level, n, i)
            # byte for byte what a context that has done nothing else writes
            fresh = cz.Context(0)
            try:
                if level.endswith("dict"):
                    with_dictionary(cz, fresh)
                want = compress(cz, fresh, level, bufs)
            finally:
                fresh.close()
            assert [f for _, f in res] == [f for _, f in want], (level, n)
            assert [r.tobytes() for r, _ in res] == [r.tobytes() for r, _ in want], (level, n)
    finally:
        shared.close()
