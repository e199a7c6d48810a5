"""cz_chain_kernel's main loop on the device: ring top-ups whose wait counts the record stores behind the prefetch, the prefetched
pieces held outside the compiler's registers, the bookkeeping between two groups of steps.  Every case goes through the C ABI into
output buffers filled with 0xA5 and is compared, frame by frame, bytes and status, with the oracle; each runs with the scheduled
asm group and with the plain C++ step (CZ_DEBUG_CHAIN_CPP_STEP)."""
import numpy as np
import pytest

import chain_loop_frames as clf
from cairo_zstd_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cz():
    import torch  # noqa: F401
    import cairo_zstd_amd as m
    return m


def _decode_and_compare(cz, frames, caps, refs, flags, shifts=None, count_wide=False):
    """One batch launch with the pre-pass on; frame i lies at a 256-aligned offset + shifts[i].  Returns the number of frames the
    chain kernel made the records of, or with count_wide the number of records of sequences of more than 32 extra bits."""
    import torch
    n = len(frames)
    shifts = shifts or [0] * n
    off, at = [], 0
    for fr, s in zip(frames, shifts):
        off.append(at + s)
        at = (at + s + len(fr) + 255) & ~255
    base = np.zeros(at + 256, np.uint8)
    for fr, o in zip(frames, off):
        base[o:o + len(fr)] = np.frombuffer(fr, np.uint8)
    out_cap = np.array(caps, np.int64)
    out_off = np.concatenate(([0], np.cumsum((out_cap + 255) & ~255)))[:-1]
    total = int(((out_cap + 255) & ~255).sum())
    dev = torch.device("cuda:0")
    t_in = torch.from_numpy(base).to(dev)
    assert t_in.data_ptr() % 256 == 0
    t = [torch.from_numpy(np.asarray(x, np.int64)).to(dev) for x in (off, [len(f) for f in frames], out_off, out_cap)]
    t_out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    t_res = torch.zeros(n * cz.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    c = cz.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        c.set_chain_arena(sum(len(f) for f in frames) * 8 + (64 << 20), min_sequences=0)
        c.set_literal_arena(sum(caps) + (16 << 20))
        c.set_debug_flags(flags)
        c.decode_batch_device(t_in.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), n, t_out.data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t_res.data_ptr())
        torch.cuda.synchronize()
        with_chain, _ = c.last_prepass_counts(n)
        wide = 0
        if count_wide:
            # the arena: per block a header {nseq << 32 | maps, ...} of 4 words, 160 words of maps, one record per sequence
            arena, used = c.debug_read_chain_arena(sum(len(f) for f in frames) * 8 + (64 << 20))
            at = 64
            while at < used and int(arena[at] >> 32):
                nseq = int(arena[at] >> 32)
                wide += int((arena[at + 164:at + 164 + nseq] >> np.uint64(63)).sum())
                at += 164 + nseq
    finally:
        c.close()
    res = t_res.cpu().numpy().view(cz.RESULT_DTYPE)
    out = t_out.cpu().numpy()
    bad = []
    for i, ref in enumerate(refs):
        got = out[int(out_off[i]):int(out_off[i]) + len(ref)]
        if int(res["status"][i]) != 0 or int(res["bytes_produced"][i]) != len(ref) or int(res["bytes_consumed"][i]) != len(frames[i]):
            bad.append((i, cz.status.name(res["status"][i]), int(res["bytes_produced"][i]), len(ref)))
        elif not np.array_equal(got, np.frombuffer(ref, np.uint8)):
            bad.append((i, "bytes", int(np.nonzero(got != np.frombuffer(ref, np.uint8))[0][0])))
    assert not bad, (len(bad), bad[:10])
    return wide if count_wide else with_chain


def _flags(cz, step):
    return cz.DEBUG_CHAIN_CPP_STEP if step == "cpp_step" else 0


@pytest.fixture(scope="module")
def mixed_rates():
    frames, caps = clf.mixed_rates(32)
    return frames, caps, clf.references(frames, caps)


@pytest.mark.parametrize("step", ["asm_group", "cpp_step"])
def test_slots_of_one_wave_use_their_rings_at_different_rates(cz, mixed_rates, step):
    """Config 4a frames (a top-up every fourth group), mix frames and libzstd's frames of long matches, long literal runs and far
    offsets (a top-up nearly every group, sequences of more than 32 extra bits: the wide redo right behind a top-up) side by side in
    the list, so in the slots of one wave: every top-up commits the pieces of ALL its slots, whatever each has used."""
    frames, caps, refs = mixed_rates
    assert len(frames) >= 64
    with_chain = _decode_and_compare(cz, frames, caps, refs, _flags(cz, step))
    print(f"frames with chain records: {with_chain} of {len(frames)}")
    assert with_chain >= 32, with_chain                                 # (the config 4a frames at the least: the records the execute stage used are the chain kernel's)


def test_the_long_match_frames_hold_wide_sequences(cz, mixed_rates):
    """What the case above relies on: libzstd's frames there do hold sequences of more than 32 extra bits (their records carry
    CZC_REC_WIDE), so the narrow asm group is redone wide in the middle of a block."""
    if clf.libzstd() is None:
        pytest.skip("no libzstd.so.1 on this box")
    frames, caps, refs = mixed_rates
    assert _decode_and_compare(cz, frames[2::3], caps[2::3], refs[2::3], 0, count_wide=True) > 0


@pytest.fixture(scope="module")
def alignments():
    src = []
    for kind, seed, first in (("full_4a", None, 11), ("full_4a", 0xC0FFEE, 400), ("full_4b", None, 77), ("mix", 1234, 9000)):
        b = synth.generate(kind, 16, seed=seed, first_index=first, nthreads=2)
        src.append([(b.frame(i), int(b.regen[i])) for i in range(16)])
    frames, caps, shifts = [], [], []
    for k in range(16):
        for s in src:
            frames.append(s[k][0]); caps.append(s[k][1]); shifts.append(k)
    return frames, caps, shifts, clf.references(frames, caps)


@pytest.mark.parametrize("step", ["asm_group", "cpp_step"])
def test_bitstreams_at_every_alignment(cz, alignments, step):
    """Every frame kind at each of the 16 byte positions modulo 16 (the frames lie at 256-aligned offsets + 0 .. 15 in a 256-aligned
    buffer, which moves the start and the end of every bitstream alike): the first and the last piece of a stream are the ones a
    lane puts together byte by byte, and a stream of more than 512 bytes commits a piece to the ring's last 16 bytes, the ones
    mirrored in front of the ring."""
    frames, caps, shifts, refs = alignments
    assert sorted(set(shifts)) == list(range(16))
    ends, long_streams = set(), set()
    for fr, s in zip(frames, shifts):
        for t, at, body in clf.walk_blocks(fr)[0]:
            if t == 2:
                ends.add((s + at + body) % 16)                          # a sequences section, hence its bitstream, ends where its block does
                if body >= 8192:
                    long_streams.add(s)
    assert ends == set(range(16)) and long_streams == set(range(16)), (sorted(ends), sorted(long_streams))
    _decode_and_compare(cz, frames, caps, refs, _flags(cz, step), shifts)


@pytest.fixture(scope="module")
def refills():
    b = synth.generate("mix", 256, first_index=31000, nthreads=2)
    frames, caps = [b.frame(i) for i in range(b.n)], [int(r) for r in b.regen]
    L = clf.libzstd()
    n_small = 0
    if L is not None:                                                   # (only this leg needs the box's libzstd)
        f2, c2 = clf.many_small_blocks(L, 64, 200)
        n_small = sum(sum(1 for t, _, _ in clf.walk_blocks(f)[0] if t == 2) for f in f2)
        assert n_small > 10240 + 1024                                   # 256 CUs x 40 slots, and the blocks 1 024 waves can be handed while the others start
        frames = [f for pair in zip(frames[:64], f2) for f in pair] + frames[64:]
        caps = [x for pair in zip(caps[:64], c2) for x in pair] + caps[64:]
    return frames, caps, clf.references(frames, caps)


@pytest.mark.parametrize("step", ["asm_group", "cpp_step"])
def test_slots_take_block_after_block(cz, refills, step):
    """Multi-block mix frames and, from libzstd, frames of 200 small blocks each — more blocks with sequences than the launch has
    slots: a slot whose chain ends takes the next block while its neighbours are in mid-stream, and nothing prefetched for the
    block it had may reach the ring of the new one."""
    frames, caps, refs = refills
    assert sum(len(clf.walk_blocks(f)[0]) for f in frames[-192:]) > 192  # the mix frames have several blocks
    _decode_and_compare(cz, frames, caps, refs, _flags(cz, step))
