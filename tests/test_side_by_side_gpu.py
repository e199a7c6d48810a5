"""Side by side (far-offset batches), cz_wexec_kernel and cz_execute_frames_kernel share a batch's frames, and a wave of the latter on
an even CU may leave its CU to the former (the gate at the top of cz_execute_frames_kernel).  These tests decode small batches,
batches of which cz_scan_kernel lists little or nothing for cz_wexec_kernel, and the worst placement (DEBUG_EXEC_LEAVE: every wave
takes the leave branch), and check every frame against the oracle.  Output and result records are poisoned before every launch,
so a frame that no kernel decoded fails instead of passing with what the buffers held before.  Each configuration runs once."""
import os

import numpy as np
import pytest

import oracle
from conftest import add_checksum, corpus_pairs

pytestmark = pytest.mark.gpu

OUT_POISON, RESULT_POISON = 0xA5, 0xFF


@pytest.fixture(scope="module")
def cz():
    import torch  # noqa: F401
    import cairo_zstd_amd as m
    assert os.path.exists(m._lib.LIB_PATH), "libcairo_zstd_amd.so missing: run __graft_entry__.build()"
    return m


def _context(cz, verify=False, force=False, cus=0, flags=0, early=False):
    c = cz.Context(0)
    c.set_chain_arena(512 << 20, min_sequences=0)
    c.set_literal_arena(256 << 20)
    c.set_verify_checksum(verify)
    if force or cus:                                                     # (else cz_wexec_kernel as a context has it by default: on, auto)
        c.set_wexec_kernel(True, cus=cus, force=force)
    c.set_debug_flags(flags)
    if early:
        c.set_early_execute(True)
    return c


def _decode_device(cz, ctx, frames, caps):
    """decode_batch_device on torch buffers, the output filled with OUT_POISON and the results with RESULT_POISON first."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(frames)
    lens = np.array([len(f) for f in frames], dtype=np.uint64)
    in_off = np.zeros(n, dtype=np.uint64)
    in_off[1:] = np.cumsum(lens[:-1])
    cap = np.array(caps, dtype=np.uint64)
    pad = (cap + np.uint64(255)) // np.uint64(256) * np.uint64(256)
    out_off = np.zeros(n, dtype=np.uint64)
    out_off[1:] = np.cumsum(pad[:-1])
    total = int(pad.sum())

    def d64(a):
        return torch.from_numpy(a.view(np.int64).copy()).to(dev)
    d_in = torch.from_numpy(np.frombuffer(b"".join(frames) + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
    d_in_off, d_in_len, d_out_off, d_cap = d64(in_off), d64(lens), d64(out_off), d64(cap)
    d_out = torch.full((max(total, 1),), OUT_POISON, dtype=torch.uint8, device=dev)
    d_res = torch.full((n * cz.RESULT_DTYPE.itemsize,), RESULT_POISON, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.decode_batch_device(d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), n, d_out.data_ptr(), d_out_off.data_ptr(),
                            d_cap.data_ptr(), d_res.data_ptr())
    ctx.synchronize()
    res = np.frombuffer(d_res.cpu().numpy().tobytes(), dtype=cz.RESULT_DTYPE)
    out = d_out.cpu().numpy()
    return [(res[i], out[int(out_off[i]): int(out_off[i]) + min(int(res[i]["bytes_produced"]), int(cap[i]))].tobytes()) for i in range(n)]


def _refs(frames, caps):
    return [oracle.decode_frame(fr, cap=cap) for fr, cap in zip(frames, caps)]


def _check(cz, refs, got, verify, label):
    """Status, bytes, bytes_consumed, blocks_decoded and the checksum fields of every frame against the oracle; with verify on,
    RESULT_CHECKSUM_COMPUTED / RESULT_CHECKSUM_MATCH and the calculated checksum against oracle.xxh64."""
    bad = []
    for i, ((st, ref, info), (r, out)) in enumerate(zip(refs, got)):
        if int(r["status"]) != st:
            bad.append(f"{label}[{i}] status {cz.status.name(r['status'])} != oracle {cz.status.name(st)}")
            continue
        if st != 0:
            continue
        flags = int(r["flags"])
        if out != ref or int(r["bytes_produced"]) != len(ref):
            bad.append(f"{label}[{i}] output ({int(r['bytes_produced'])} bytes, oracle {len(ref)})")
        elif int(r["bytes_consumed"]) != info["consumed"] or int(r["blocks_decoded"]) != info["blocks"]:
            bad.append(f"{label}[{i}] consumed/blocks {int(r['bytes_consumed'])}/{int(r['blocks_decoded'])} vs {info['consumed']}/{info['blocks']}")
        elif bool(flags & cz.RESULT_HAS_CHECKSUM) != info["has_checksum"] or (info["has_checksum"] and int(r["checksum_from_data"]) != info["checksum"]):
            bad.append(f"{label}[{i}] checksum field")
        elif verify and info["has_checksum"]:
            want = oracle.xxh64(ref) & 0xFFFFFFFF
            if not flags & cz.RESULT_CHECKSUM_COMPUTED or int(r["calculated_checksum"]) != want or bool(flags & cz.RESULT_CHECKSUM_MATCH) != (want == info["checksum"]):
                bad.append(f"{label}[{i}] XXH64 flags {flags:#x} calculated {int(r['calculated_checksum']):#x} want {want:#x}")
    assert not bad, "\n".join(bad[:20]) + f"\n({len(bad)} of {len(refs)} frames wrong)"


def _full_4a(n, first_index, checksum):
    """n config-4a frames (far offsets: side by side in auto mode); checksum: each with the content checksum of its content."""
    from cairo_zstd_amd import synth
    b = synth.generate("full_4a", n, first_index=first_index)
    frames, caps = [b.frame(i) for i in range(n)], [int(r) + 16 for r in b.regen]
    if checksum:
        frames = [add_checksum(z, oracle.decode_frame(z, cap=cap)[1]) for z, cap in zip(frames, caps)]
    return frames, caps


@pytest.fixture(scope="module")
def checksummed_4a():
    frames, caps = _full_4a(300, 60001, checksum=True)
    return frames, caps, _refs(frames, caps)


def _small_frames(count):
    """Frames of one block and at most 1 000 bytes of content: under 340 sequences, so under CZ_WX_MIN_UNITS (512) chain units
    (4 + 160 + one per sequence) — never listed."""
    from cairo_zstd_amd import synth
    out = [(z, len(orig) + 16) for _, z, orig in corpus_pairs(max_orig=1000) if len(orig) > 0]
    b = synth.generate("mix", 60, first_index=321, nthreads=2)
    out += [(b.frame(i), int(b.regen[i]) + 8) for i in range(b.n) if 0 < b.regen[i] <= 1000]
    out = [(z, cap) for z, cap in out if oracle.decode_frame(z, cap=cap)[2]["blocks"] == 1]
    out = out[::3] + out[1::3] + out[2::3]                               # corpus and mix frames interleaved
    return [z for z, _ in out[:count]], [c for _, c in out[:count]]


def _damaged(z: bytes, seed: int):
    rng = np.random.default_rng(seed)
    out = [z[: len(z) // 2], z[:-1], z[:5], z + b"\x00"]
    for _ in range(4):
        a = bytearray(z)
        a[int(rng.integers(0, len(a)))] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(a))
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 8, 64, 300])
def test_nothing_listed_auto_mode_loses_no_frame(cz, checksummed_4a, n):
    """Checksummed config-4a frames with verify on, cz_wexec_kernel in its default (auto) mode: the batch's far offsets put the
    execute stage side by side, but cz_scan_kernel lists no frame (a content checksum to verify), so cz_wexec_kernel returns
    before it counts itself in.  No wave of cz_execute_frames_kernel may wait for it or leave, and every frame is decoded."""
    frames, caps, refs = checksummed_4a
    frames, caps, refs = frames[:n], caps[:n], refs[:n]
    c = _context(cz, verify=True)
    try:
        got = _decode_device(cz, c, frames, caps)
        assert c.last_wexec_counts()[0] == 0, c.last_wexec_counts()
        wexec_in, left, waited = c.last_side_counts()
        assert wexec_in == 0 and left == 0 and waited == 0, (wexec_in, left, waited)
        _check(cz, refs, got, True, f"n={n}")
    finally:
        c.close()


@pytest.mark.parametrize("n", [1, 2, 8])
def test_nothing_listed_forced_small_frames(cz, n):
    """cz_wexec_kernel forced side by side on frames too small to be listed: every frame decoded, no wave left."""
    frames, caps = _small_frames(n)
    assert len(frames) == n
    c = _context(cz, force=True)
    try:
        got = _decode_device(cz, c, frames, caps)
        assert c.last_wexec_counts()[0] == 0, c.last_wexec_counts()
        assert c.last_side_counts()[1] == 0, c.last_side_counts()
        _check(cz, _refs(frames, caps), got, False, f"small n={n}")
    finally:
        c.close()


@pytest.mark.parametrize("n", [1, 8])
def test_nothing_listed_forced_checksummed(cz, checksummed_4a, n):
    """cz_wexec_kernel forced side by side on checksummed config-4a frames with verify on: nothing listed, every frame decoded and
    its XXH64 computed, no wave left."""
    frames, caps, refs = checksummed_4a
    c = _context(cz, verify=True, force=True)
    try:
        got = _decode_device(cz, c, frames[:n], caps[:n])
        assert c.last_wexec_counts()[0] == 0, c.last_wexec_counts()
        assert c.last_side_counts()[1] == 0, c.last_side_counts()
        _check(cz, refs[:n], got, True, f"checksummed n={n}")
    finally:
        c.close()


@pytest.mark.parametrize("exec_first", [False, True])
def test_some_listed_wexec_short_of_its_cus(cz, checksummed_4a, exec_first):
    """cz_wexec_kernel forced side by side and asked for more CUs than the device has (the host clamps to all of them), so its
    workgroups cannot all count themselves in while cz_execute_frames_kernel holds CUs: waves on even CUs leave after their wait.
    Batches of one or two listed config-4a frames and a few unlisted ones (small, and checksummed with verify on).  DEBUG_EXEC_FIRST
    only changes the order in which the host submits the two kernels, not where the dispatcher places them."""
    from cairo_zstd_amd import DEBUG_EXEC_FIRST
    plain, plain_caps = _full_4a(2, 61001, checksum=False)
    ck, ck_caps, ck_refs = checksummed_4a
    small, small_caps = _small_frames(6)
    batches = [
        (plain[:1] + small[:1], plain_caps[:1] + small_caps[:1], 1),
        (plain[:1] + ck[:2], plain_caps[:1] + ck_caps[:2], 1),
        (plain + small[:3] + ck[2:5], plain_caps + small_caps[:3] + ck_caps[2:5], 2),
        (small[3:6] + plain + ck[5:8], small_caps[3:6] + plain_caps + ck_caps[5:8], 2),
    ]
    c = _context(cz, verify=True, force=True, cus=100000, flags=DEBUG_EXEC_FIRST if exec_first else 0)
    try:
        for k, (frames, caps, listed) in enumerate(batches):
            got = _decode_device(cz, c, frames, caps)
            _check(cz, _refs(frames, caps), got, True, f"batch {k}")
            assert c.last_wexec_counts()[0] == listed, (k, c.last_wexec_counts())
            assert c.last_side_counts()[1] < len(frames), (k, c.last_side_counts())   # never every wave
    finally:
        c.close()


def _mixed_batch():
    from cairo_zstd_amd import synth
    frames, caps = [], []
    for kind, n in (("full_4b", 3), ("mix", 120)):
        b = synth.generate(kind, n, first_index=8008)
        frames += [b.frame(i) for i in range(n)]
        caps += [int(r) + 16 for r in b.regen]
    for name, z, orig in corpus_pairs():
        frames.append(z)
        caps.append(len(orig) + 32)
    for idx, (name, z, orig) in enumerate(corpus_pairs(max_orig=4000)[:10]):
        for m in _damaged(z, 500 + idx):
            frames.append(m)
            caps.append(len(orig) * 2 + 4096)
    return frames, caps


def _check_every_wave_leaves(cz, c, frames, caps, label):
    got = _decode_device(cz, c, frames, caps)
    _check(cz, _refs(frames, caps), got, False, label)
    left = c.last_side_counts()[1]
    grid = min(len(frames), max(c.execute_grid()))
    assert left < max(grid, 1), (label, left, grid)                      # one wave stays ...
    if len(frames) > 1:
        assert left >= 1, (label, left)                                  # ... and the others took the leave branch


@pytest.mark.parametrize("n", [1, 8, 300])
def test_every_wave_leaves_config_4a(cz, n):
    """DEBUG_EXEC_LEAVE: every wave of cz_execute_frames_kernel takes the leave branch, as if it were on an even CU that
    cz_wexec_kernel never met.  The wave whose leave would make the count reach the grid stays and executes what is left."""
    from cairo_zstd_amd import DEBUG_EXEC_LEAVE
    frames, caps = _full_4a(n, 62001, checksum=False)
    c = _context(cz, force=True, flags=DEBUG_EXEC_LEAVE)
    try:
        _check_every_wave_leaves(cz, c, frames, caps, f"4a n={n}")
    finally:
        c.close()


@pytest.mark.parametrize("early", [False, True])
def test_every_wave_leaves_mixed_batch(cz, early):
    """DEBUG_EXEC_LEAVE on config 4b, corpus-like, reference-corpus and damaged frames, with the one-launch arrangement and with
    set_early_execute(True) (the gated launch is then args.early == 2, behind the early launches)."""
    from cairo_zstd_amd import DEBUG_EXEC_LEAVE
    frames, caps = _mixed_batch()
    c = _context(cz, force=True, flags=DEBUG_EXEC_LEAVE, early=early)
    try:
        _check_every_wave_leaves(cz, c, frames, caps, f"mixed early={early}")
    finally:
        c.close()


@pytest.mark.parametrize("leave", [False, True])
def test_back_to_back_batches_keep_their_own_results(cz, leave):
    """Two different batches of the same size (checksummed config 4a, verify on, nothing listed), one after the other on one
    context, through decode_batch_host (whose staging buffers are reused from call to call) and then decode_batch_device: the
    second batch's records and bytes are its own, not the first's; also with every wave taking the leave branch."""
    flags = cz.DEBUG_EXEC_LEAVE if leave else 0
    first, first_caps = _full_4a(3, 63001, checksum=True)
    second, second_caps = _full_4a(3, 63101, checksum=True)
    refs1, refs2 = _refs(first, first_caps), _refs(second, second_caps)
    assert all(a[1] != b[1] for a, b in zip(refs1, refs2))
    c = _context(cz, verify=True, flags=flags)
    try:
        _check(cz, refs1, cz.decode_batch_host(first, first_caps, c), True, "host first")
        _check(cz, refs2, cz.decode_batch_host(second, second_caps, c), True, "host second")
        _check(cz, refs1, _decode_device(cz, c, first, first_caps), True, "device first")
        _check(cz, refs2, _decode_device(cz, c, second, second_caps), True, "device second")
    finally:
        c.close()
