"""CPU twin of test_chain_loop_gpu.py's first case: cz_chain_kernel's main loop (the plain C++ of the ring top-up and of the step,
which the device build mirrors in inline asm) on the SIMT emulator of tests/emu, a stand-alone program built with
AddressSanitizer and UBSan, against the oracle."""
import chain_loop_frames as clf
import emu_runner
from cairo_zstd_amd import status


def test_emu_slots_of_one_wave_use_their_rings_at_different_rates():
    """Mix frames and (with a libzstd on the box) frames of long matches, long literal runs and far offsets — sequences of more than
    32 extra bits among ordinary ones — in the slots of one wave, topped up together whatever each has used.  (The config 4a frames
    of the device test are left out: one is a minute on the emulator.)"""
    frames, caps = clf.mixed_rates(1, small=True)
    refs = clf.references(frames, caps)
    res = emu_runner.run(frames, caps, chain_bytes=8 << 20, lit_bytes=4 << 20, exec_kernel=True)
    bad = [(i, status.name(r["status"]), len(out), len(ref)) for i, ((r, out), ref) in enumerate(zip(res, refs)) if int(r["status"]) != 0 or out != ref]
    assert not bad, bad
