"""cz_context_set_dictionaries on the MI355X: batches whose frames pick their dictionary by the Dictionary_ID of their header
(tests/golden/multidict, made by scripts/gen_multidict_vectors.py).  Run with `pytest -m gpu`."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import multidict_data as md
from conftest import corpus_pairs

pytestmark = pytest.mark.gpu
POISON = 0xEE
PREPASS = {"off": (0, 0), "chain": (64 << 20, 0), "chain_and_literals": (256 << 20, 128 << 20)}


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
def dicts(cz, ctx):
    """name -> cz.Dictionary on the module's context, for all five dictionaries."""
    out = {n: cz.Dictionary(ctx, md.dict_bytes(n)) for n in md.MANIFEST["dictionaries"]}
    for n, d in out.items():
        assert d.id == md.MANIFEST["dictionaries"][n]["id"], n
    yield out
    ctx.set_dictionary(None)
    for d in out.values():
        d.close()


def registered(dicts):
    return [dicts[n] for n in md.REGISTERED]


def set_prepass(ctx, mode):
    chain, lit = PREPASS[mode]
    ctx.set_chain_arena(chain, min_sequences=0)
    ctx.set_literal_arena(lit)


class Launch:
    """Device buffers for one batch; run() fills every output region with POISON, launches, and returns [(result record, whole
    output region)].  The same buffers on every run, so that a repeated launch can be replayed as a graph."""

    def __init__(self, cz, zs, caps):
        import torch
        dev = torch.device("cuda:0")
        self.cz, self.n = cz, len(zs)
        lens = np.array([len(z) for z in zs], dtype=np.int64)
        in_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        self.caps = np.array(caps, dtype=np.int64)
        pad = (self.caps + 255) // 256 * 256
        self.out_off = np.concatenate([[0], np.cumsum(pad)[:-1]]).astype(np.int64)
        self.t_in = torch.from_numpy(np.frombuffer(b"".join(zs) + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        self.t_off, self.t_len = torch.from_numpy(in_off).to(dev), torch.from_numpy(lens).to(dev)
        self.t_ooff, self.t_ocap = torch.from_numpy(self.out_off).to(dev), torch.from_numpy(self.caps).to(dev)
        self.t_out = torch.empty((int(pad.sum()),), dtype=torch.uint8, device=dev)
        self.t_res = torch.zeros(self.n * cz.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)

    def run(self, ctx):
        import torch
        self.t_out.fill_(POISON)
        self.t_res.zero_()
        torch.cuda.synchronize()
        ctx.decode_batch_device(self.t_in.data_ptr(), self.t_off.data_ptr(), self.t_len.data_ptr(), self.n, self.t_out.data_ptr(),
                                self.t_ooff.data_ptr(), self.t_ocap.data_ptr(), self.t_res.data_ptr())
        torch.cuda.synchronize()
        res, out = self.t_res.cpu().numpy().view(self.cz.RESULT_DTYPE), self.t_out.cpu().numpy().tobytes()
        return [(res[i], out[int(self.out_off[i]): int(self.out_off[i] + self.caps[i])]) for i in range(self.n)]


def decode_poisoned(cz, ctx, zs, caps):
    return Launch(cz, zs, caps).run(ctx)


def check(cz, batch, got, verify=False, unknown_ok=True):
    """Known frames bit-exact with the rest of their region untouched; frames naming an unregistered ID CZ_E_DICT_UNKNOWN with
    the ID in detail[0], nothing produced, their region untouched."""
    bad = []
    for i, (f, (r, region)) in enumerate(zip(batch, got)):
        st, n = int(r["status"]), int(r["bytes_produced"])
        if f.dictionary == md.UNREGISTERED and unknown_ok:
            if st != cz.status.CZ_E_DICT_UNKNOWN or int(r["detail"][0]) != f.id or n != 0:
                bad.append(f"[{i}] {f}: {cz.status.name(st)} detail {int(r['detail'][0]):#x} produced {n}")
            elif region != bytes([POISON]) * len(region):
                bad.append(f"[{i}] {f}: output region written")
            continue
        if st != 0:
            bad.append(f"[{i}] {f}: {cz.status.name(st)} detail {r['detail']}")
        elif not f.matches(region[:n]):
            bad.append(f"[{i}] {f}: output differs")
        elif region[n:] != bytes([POISON]) * (len(region) - n):
            bad.append(f"[{i}] {f}: bytes written past the frame's output")
        elif verify and f.meta["has_checksum"] and not (r["flags"] & cz.RESULT_CHECKSUM_COMPUTED and r["flags"] & cz.RESULT_CHECKSUM_MATCH
                                                       and int(r["calculated_checksum"]) == int(r["checksum_from_data"])):
            bad.append(f"[{i}] {f}: checksum flags {int(r['flags'])}")
        elif not verify and r["flags"] & cz.RESULT_CHECKSUM_COMPUTED:
            bad.append(f"[{i}] {f}: checksum computed with verification off")
    assert not bad, "\n".join(bad[:20]) + f"\n({len(bad)} of {len(batch)} frames)"


def run(cz, ctx, batch, **kw):
    got = decode_poisoned(cz, ctx, [f.zst for f in batch], [f.orig_len + 64 for f in batch])
    check(cz, batch, got, **kw)
    return got


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("prepass", sorted(PREPASS))
def test_mixed_batch_of_four_dictionaries(cz, ctx, dicts, prepass, verify):
    """~2 000 shuffled frames: every frame of the four registered dictionaries, the no-ID frames of dict_a (the no-ID
    dictionary) and plain frames, in one launch; every output bit-exact, computed checksums matching."""
    base = md.registered_frames() + [f for f in md.noid_frames() if f.dictionary == "dict_a"] + md.plain_frames()
    batch = base * (2000 // len(base) + 1)
    random.Random(7).shuffle(batch)
    set_prepass(ctx, prepass)
    ctx.set_verify_checksum(verify)
    ctx.set_dictionaries(registered(dicts), no_id=dicts["dict_a"])
    try:
        run(cz, ctx, batch, verify=verify)
    finally:
        ctx.set_dictionaries([])
        ctx.set_verify_checksum(False)
        set_prepass(ctx, "off")


@pytest.mark.parametrize("prepass", sorted(PREPASS))
def test_unknown_ids_fail_alone(cz, ctx, dicts, prepass):
    """Frames naming the unregistered fifth dictionary — x_raw is Raw blocks only, which the pre-pass would finish by itself —
    are CZ_E_DICT_UNKNOWN with the ID and leave their region untouched; their neighbours decode.  Header errors keep their
    precedence: a frame cut inside its ID field is CZ_E_FH_DICT_ID_READ, a skippable frame CZ_E_FH_SKIP_FRAME."""
    known = md.registered_frames() + md.plain_frames()
    batch = []
    for k in range(6):
        for f in known:
            batch.append(f)
            batch.append(md.unknown_frames()[(k + len(batch)) % len(md.unknown_frames())])
    set_prepass(ctx, prepass)
    ctx.set_dictionaries(registered(dicts))
    try:
        got = run(cz, ctx, batch)
        assert sum(int(r["status"]) == cz.status.CZ_E_DICT_UNKNOWN for r, _ in got) == len(batch) // 2
        assert any(f.name == "x_raw" for f in batch)
        cut = md.Frame("x_small_0").zst[:7]                             # magic, descriptor, 2 of its 4 ID bytes
        skip = bytes.fromhex("502a4d18") + (3).to_bytes(4, "little") + b"abc"
        res = decode_poisoned(cz, ctx, [cut, skip, md.Frame("c_small_0").zst], [64, 64, 1024])
        assert int(res[0][0]["status"]) == cz.status.CZ_E_FH_DICT_ID_READ == cz.read_frame_header(cut)[0]
        assert int(res[1][0]["status"]) == cz.status.CZ_E_FH_SKIP_FRAME
        assert int(res[2][0]["status"]) == 0 and md.Frame("c_small_0").matches(res[2][1][:int(res[2][0]["bytes_produced"])])
    finally:
        ctx.set_dictionaries([])
        set_prepass(ctx, "off")


@pytest.mark.parametrize("prepass", ["off", "chain_and_literals"])
def test_no_id_dictionary(cz, ctx, dicts, prepass):
    """Frames without an ID field start from no_id_dict: with the dictionary they were made with they decode; with none,
    plain frames still decode and the dictionary frames without an ID do not give their original."""
    set_prepass(ctx, prepass)
    try:
        for f in md.noid_frames():
            ctx.set_dictionaries(registered(dicts), no_id=dicts[f.dictionary])
            run(cz, ctx, [f] + md.plain_frames() + md.registered_frames())
        ctx.set_dictionaries(registered(dicts))
        run(cz, ctx, md.plain_frames() + md.registered_frames())
        for f, (r, region) in zip(md.noid_frames(), decode_poisoned(cz, ctx, [f.zst for f in md.noid_frames()], [f.orig_len + 64 for f in md.noid_frames()])):
            assert int(r["status"]) != 0 or not f.matches(region[:int(r["bytes_produced"])]), f
    finally:
        ctx.set_dictionaries([])
        set_prepass(ctx, "off")


def test_argument_errors_keep_the_previous_setting(cz, ctx, dicts):
    """CZ_E_INVALID_ARG for every rule of cz_context_set_dictionaries; after each, the setting before it still decodes."""
    L = cz.lib()
    reg = registered(dicts)
    ctx.set_dictionaries(reg[:2], no_id=dicts["dict_a"])             # dict_a, dict_b
    sample = [f for f in md.registered_frames() if f.dictionary in ("dict_a", "dict_b")] + [md.Frame("a_noid")] + md.plain_frames()
    sample_unknown = [f for f in md.registered_frames() if f.dictionary == "dict_c"][:2]
    other = cz.Context(0)
    zero = bytearray(md.dict_bytes("dict_c"))
    zero[4:8] = b"\0\0\0\0"
    from conftest import GOLDEN
    same_a, same_b = (cz.Dictionary(ctx, open(os.path.join(GOLDEN, "dict", n), "rb").read()) for n in ("dict.bin", "dict_hist.bin"))
    assert same_a.id == same_b.id != 0
    d_zero, d_other = cz.Dictionary(ctx, bytes(zero)), cz.Dictionary(other, md.dict_bytes("dict_c"))
    assert d_zero.id == 0
    arr = lambda ds: (C.c_void_p * len(ds))(*[d._h.value if d is not None else None for d in ds])
    cases = {
        "NULL list with k > 0": lambda: L.cz_context_set_dictionaries(ctx._h, None, 2, None),
        "NULL entry": lambda: L.cz_context_set_dictionaries(ctx._h, arr([reg[2], None]), 2, None),
        "dictionary of another context": lambda: L.cz_context_set_dictionaries(ctx._h, arr([reg[2], d_other]), 2, None),
        "no_id of another context": lambda: L.cz_context_set_dictionaries(ctx._h, arr([reg[2]]), 1, d_other._h),
        "listed dictionary with ID 0": lambda: L.cz_context_set_dictionaries(ctx._h, arr([reg[2], d_zero]), 2, None),
        "two dictionaries with one ID": lambda: L.cz_context_set_dictionaries(ctx._h, arr([same_a, same_b]), 2, None),
        "more than CZ_MAX_DICTIONARIES": lambda: L.cz_context_set_dictionaries(ctx._h, arr(reg[2:3] * 1025), 1025, None),
    }
    try:
        for what, call in cases.items():
            assert call() == cz.status.CZ_E_INVALID_ARG, what
            run(cz, ctx, sample)
            for r, _ in decode_poisoned(cz, ctx, [f.zst for f in sample_unknown], [f.orig_len + 64 for f in sample_unknown]):
                assert int(r["status"]) == cz.status.CZ_E_DICT_UNKNOWN, what
        with pytest.raises(cz.CzError):
            ctx.set_dictionaries([reg[2], None])
        run(cz, ctx, sample)
        ctx.set_dictionaries([d_zero][:0], no_id=d_zero)                # (ID 0 is allowed as the no-ID dictionary)
    finally:
        ctx.set_dictionaries([])
        for d in (same_a, same_b, d_zero, d_other):
            d.close()
        other.close()


def test_switching_between_the_two_calls(cz, ctx, dicts):
    """set_dictionaries -> set_dictionary(d) (every frame starts from d, whatever ID it names) -> clear: after clearing,
    ordinary frames decode as before, and an ID the context never heard of is no error."""
    reg = registered(dicts)
    x_raw = md.Frame("x_raw")
    ctx.set_dictionaries(reg)
    run(cz, ctx, md.registered_frames() + [x_raw])
    ctx.set_dictionary(dicts["dict_b"])
    b_frames = [f for f in md.registered_frames() if f.dictionary == "dict_b"]
    run(cz, ctx, b_frames + md.plain_frames())
    got = decode_poisoned(cz, ctx, [x_raw.zst, md.Frame("c_small_0").zst], [x_raw.orig_len + 64, 1024])
    assert int(got[0][0]["status"]) == 0 and x_raw.matches(got[0][1][:x_raw.orig_len])       # the ID is ignored
    assert int(got[1][0]["status"]) != cz.status.CZ_E_DICT_UNKNOWN
    ctx.set_dictionaries([])
    pairs = corpus_pairs()[:12]
    for (name, z, orig), (r, out) in zip(pairs, cz.decode_batch_host([z for _, z, _ in pairs], [len(o) + 32 for _, _, o in pairs], ctx)):
        assert int(r["status"]) == 0 and out == orig, name
    got = decode_poisoned(cz, ctx, [x_raw.zst], [x_raw.orig_len + 64])
    assert int(got[0][0]["status"]) == 0 and x_raw.matches(got[0][1][:x_raw.orig_len])


def test_swapping_dictionary_sets_under_graph_replay(cz, dicts):
    """With graph replay on, a repeated launch is captured and replayed; swapping the set of dictionaries between launches
    changes the context, so the next launches decode with the new table, not the captured one."""
    import torch
    c = cz.Context(0, torch.cuda.current_stream().cuda_stream)
    own = {n: cz.Dictionary(c, md.dict_bytes(n)) for n in md.REGISTERED}
    try:
        c.set_chain_arena(64 << 20, min_sequences=0)
        c.set_literal_arena(64 << 20)
        c.set_graph_replay(True)
        batch = md.registered_frames() * 8
        set1, set2 = ("dict_a", "dict_b"), ("dict_c", "dict_d")
        launch = Launch(cz, [f.zst for f in batch], [f.orig_len + 64 for f in batch])
        for names in (set1, set2, set1):
            c.set_dictionaries([own[n] for n in names])
            replays = []
            for _ in range(3):
                got = launch.run(c)
                replays.append(c.last_launch_was_replay())
                for f, (r, region) in zip(batch, got):
                    if f.dictionary in names:
                        assert int(r["status"]) == 0 and f.matches(region[:int(r["bytes_produced"])]), (names, f)
                    else:
                        assert int(r["status"]) == cz.status.CZ_E_DICT_UNKNOWN and int(r["detail"][0]) == f.id, (names, f)
                        assert region == bytes([POISON]) * len(region), (names, f)
            assert replays[0] is False or not cz.graph_replay_available(), names
            if cz.graph_replay_available():
                assert replays[1:] == [True, True], (names, replays)
    finally:
        c.set_dictionaries([])
        for d in own.values():
            d.close()
        c.close()


def test_decode_stream_across_dictionaries(cz, ctx, dicts):
    """decode_stream of one stream whose frames come from different dictionaries, a skippable frame between them."""
    parts = [md.Frame(n) for n in ("a_small_0", "b_multi_l3", "c_small_1", "d_multi_l19", "plain_0", "a_noid")]
    skip = bytes.fromhex("512a4d18") + (5).to_bytes(4, "little") + b"hello"
    stream = parts[0].zst + parts[1].zst + skip + parts[2].zst + parts[3].zst + skip + parts[4].zst + parts[5].zst
    ctx.set_dictionaries(registered(dicts), no_id=dicts["dict_a"])
    try:
        out = cz.decode_stream(stream, ctx)
    finally:
        ctx.set_dictionaries([])
    assert out == b"".join(f.orig for f in parts)
