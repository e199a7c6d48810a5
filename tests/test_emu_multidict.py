"""cz_context_set_dictionaries on the CPU SIMT emulator (tests/emu/emu_multidict.cpp, ASan + UBSan): the dictionaries parsed by
cz_dict_setup_kernel, the table filled as the host library fills it, then cz_decode_frames_kernel — alone, and behind the whole
pre-pass (cz_scan_kernel, cz_chain_kernel, the literal and copy kernels).  No GPU needed."""
import pytest

import emu_multidict_runner
import multidict_data as md

STATUS_DICT_UNKNOWN = 907
PREPASS = {"off": (0, 0), "chain_and_literals": (32 << 20, 16 << 20)}


@pytest.mark.xdist_group(name="emu_multidict")
@pytest.mark.parametrize("prepass", sorted(PREPASS))
def test_emu_mixed_dictionaries_and_unknown_ids(prepass):
    """One batch: every frame of the four registered dictionaries, a frame without an ID (the no-ID dictionary is dict_a), plain
    frames, and frames naming the unregistered fifth dictionary — x_raw is Raw blocks only, which the pre-pass would otherwise
    finish by itself.  Known frames are bit-exact; unknown ones are CZ_E_DICT_UNKNOWN with the ID, their output untouched."""
    from cairo_zstd_amd import status
    assert status.CZ_E_DICT_UNKNOWN == STATUS_DICT_UNKNOWN
    known = md.registered_frames() + [f for f in md.noid_frames() if f.dictionary == "dict_a"] + md.plain_frames()
    unknown = md.unknown_frames()
    batch = []
    for i, f in enumerate(known):                                       # unknown frames between known ones
        batch.append(f)
        if i % 4 == 1 and unknown:
            batch.append(unknown.pop())
    batch += unknown
    caps = [f.orig_len + 64 for f in batch]
    chain, lit = PREPASS[prepass]
    got = emu_multidict_runner.run([f.zst for f in batch], caps, [md.dict_path(n) for n in md.REGISTERED], no_id=md.dict_path("dict_a"),
                                   chain_bytes=chain, lit_bytes=lit, verify=True)
    nknown = nunknown = 0
    for f, cap, (r, region) in zip(batch, caps, got):
        if f.dictionary == md.UNREGISTERED:
            assert int(r["status"]) == STATUS_DICT_UNKNOWN, (f, int(r["status"]))
            assert int(r["detail"][0]) == md.UNKNOWN_ID and int(r["bytes_produced"]) == 0, f
            assert region == b"\xee" * cap, f"{f}: output region written"
            nunknown += 1
        else:
            assert int(r["status"]) == 0, (f, int(r["status"]))
            assert f.matches(region[:int(r["bytes_produced"])]), f
            assert region[int(r["bytes_produced"]):] == b"\xee" * (cap - int(r["bytes_produced"])), f
            if f.meta["has_checksum"]:
                assert r["flags"] & 8 and int(r["calculated_checksum"]) == int(r["checksum_from_data"]), f
            nknown += 1
    assert nunknown == len(md.unknown_frames()) and nknown == len(known)
