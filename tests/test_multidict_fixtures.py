"""The committed several-dictionaries fixtures (tests/golden/multidict): what their frame headers say, read with
cz_read_frame_header, is what the manifest records.  No GPU needed."""
import hashlib

import multidict_data as md


def test_multidict_fixture_headers_match_the_manifest():
    import cairo_zstd_amd as cz
    widths = set()
    for f in md.frames():
        st, fh, _ = cz.read_frame_header(f.zst)
        assert st == 0, (f, cz.status.name(st))
        assert (fh.dict_id if fh.has_dict_id else 0) == f.id, f
        assert (0, 1, 2, 4)[fh.descriptor & 3] == f.meta["id_width"], f
        assert bool(fh.descriptor & 4) == f.meta["has_checksum"], f
        if f.dictionary:
            assert f.id in (0, md.MANIFEST["dictionaries"][f.dictionary]["id"]), f
        if f.orig is not None:
            assert hashlib.sha256(f.orig).hexdigest() == f.meta["orig_sha256"], f
        widths.add(f.meta["id_width"])
    assert widths == {0, 1, 2, 4}
    ids = sorted(md.MANIFEST["dictionaries"][n]["id"] for n in md.REGISTERED)
    assert ids[0] < 256 <= ids[1] < 65536 <= ids[2] < 2 ** 31 <= ids[3]
    for n, d in md.MANIFEST["dictionaries"].items():
        raw = md.dict_bytes(n)
        assert hashlib.sha256(raw).hexdigest() == d["sha256"] and int.from_bytes(raw[4:8], "little") == d["id"], n
