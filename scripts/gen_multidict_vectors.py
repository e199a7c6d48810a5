#!/usr/bin/env python3
"""Makes the several-dictionaries fixtures under tests/golden/multidict/ with the host's libzstd (data only: trained
dictionaries, frames compressed with them, the originals, manifest.json).  Deterministic inputs; re-running it with the same
libzstd gives the same bytes, another version may give other (equally valid) ones, which is why the outputs are committed.

    dict_a..dict_d.bin   four dictionaries trained on four record families with different vocabularies, their IDs patched
                         so that they cover every width of the frame header's Dictionary_ID field: 1 byte (< 256), 2 bytes
                         (< 65536), 4 bytes (>= 65536) and 4 bytes (>= 2^31)
    dict_x.bin           a fifth dictionary that the tests never register
    <name>.zst           per registered dictionary: small records (their first block leans on the dictionary's tables and
                         content), multi-KB records at levels 3 and 19, one frame over 128 KiB (two blocks), some with the
                         content checksum; across dictionaries: frames without an ID field (ZSTD_c_dictIDFlag = 0), plain
                         frames without a dictionary, frames made with dict_x, and one frame of Raw blocks only whose header
                         names dict_x's ID
    <name>.orig          the original, where it is small (manifest.json has every original's length and sha256)
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "multidict")
ORIG_MAX = 16384                     # originals up to this size are committed next to their frames
L = C.CDLL("libzstd.so.1")
for f in ("ZDICT_trainFromBuffer", "ZSTD_compress2", "ZSTD_decompress_usingDict", "ZSTD_compressBound", "ZSTD_CCtx_loadDictionary",
          "ZSTD_CCtx_setParameter", "ZSTD_CCtx_reset"):
    getattr(L, f).restype = C.c_size_t
L.ZSTD_createCCtx.restype = C.c_void_p
L.ZSTD_createDCtx.restype = C.c_void_p
L.ZSTD_isError.restype = C.c_uint
L.ZDICT_isError.restype = C.c_uint
ZSTD_c_compressionLevel, ZSTD_c_checksumFlag, ZSTD_c_dictIDFlag = 100, 201, 202
ZSTD_reset_session_and_parameters = 3

# name -> (record family, Dictionary_ID written into the dictionary's header)
DICTS = {"a": ("users", 0xC5), "b": ("access_log", 0x9C41), "c": ("sensors", 0x00123457), "d": ("orders", 0x9ABCDEF1),
         "x": ("chat", 0x00777771)}


def record(family, rng, i):
    """One record of a family: shared field names and vocabulary (what a dictionary is for) + unique values."""
    pick = lambda words, k: " ".join(words[int(j)] for j in rng.integers(0, len(words), size=k))
    if family == "users":
        w = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel", "india", "juliet", "kilo", "lima"]
        return (f'{{"id": {i}, "user": "user_{int(rng.integers(0, 5000))}", "status": "{"active" if i % 3 else "suspended"}", '
                f'"score": {float(rng.random()):.6f}, "description": "{pick(w, int(rng.integers(20, 90)))}"}}\n').encode()
    if family == "access_log":
        paths = ["/api/v2/items", "/static/app.js", "/login", "/api/v2/cart/checkout", "/images/logo.png", "/healthz"]
        agents = ["Mozilla/5.0 (X11; Linux x86_64)", "curl/8.4.0", "python-requests/2.31", "Go-http-client/2.0"]
        return (f'10.{int(rng.integers(0, 256))}.{int(rng.integers(0, 256))}.{int(rng.integers(0, 256))} - - [12/Mar/2026:10:{i % 60:02d}:{int(rng.integers(0, 60)):02d} +0000] '
                f'"GET {paths[int(rng.integers(0, len(paths)))]}?page={int(rng.integers(0, 40))} HTTP/1.1" {[200, 200, 304, 404, 500][int(rng.integers(0, 5))]} '
                f'{int(rng.integers(100, 90000))} "-" "{agents[int(rng.integers(0, len(agents)))]}"\n').encode()
    if family == "sensors":
        kinds = ["temperature_celsius", "relative_humidity", "pressure_hectopascal", "co2_ppm", "battery_voltage"]
        return "".join(f"station-{int(rng.integers(0, 64)):03d};{kinds[int(rng.integers(0, len(kinds)))]};{float(rng.normal(20, 5)):.3f};"
                       f"2026-03-12T{i % 24:02d}:{int(rng.integers(0, 60)):02d}:00Z;quality=GOOD\n" for _ in range(int(rng.integers(3, 9)))).encode()
    if family == "orders":
        items = ["widget", "gadget", "sprocket", "flange", "gasket", "bearing", "spindle", "coupling"]
        lines = "".join(f"<line sku=\"SKU-{int(rng.integers(0, 99999)):05d}\" item=\"{items[int(rng.integers(0, len(items)))]}\" qty=\"{int(rng.integers(1, 20))}\"/>"
                        for _ in range(int(rng.integers(1, 6))))
        return (f"<order number=\"{100000 + i}\" currency=\"EUR\" customer=\"C{int(rng.integers(0, 9999)):04d}\"><shipping method=\"express\" "
                f"country=\"DE\"/>{lines}<total>{float(rng.random() * 900):.2f}</total></order>\n").encode()
    w = ["hey", "thanks", "see you tomorrow", "sounds good", "lol", "on my way", "meeting moved", "lunch?"]
    return f"[chat room={int(rng.integers(0, 30))} from=@member{int(rng.integers(0, 800))}] {pick(w, int(rng.integers(3, 12)))}\n".encode()


def train(family, rng, dict_id):
    samples = [record(family, rng, i) for i in range(600)]
    sizes = (C.c_size_t * len(samples))(*[len(s) for s in samples])
    dcap = 8192
    buf = C.create_string_buffer(dcap)
    n = L.ZDICT_trainFromBuffer(buf, C.c_size_t(dcap), b"".join(samples), sizes, C.c_uint(len(samples)))
    assert not L.ZDICT_isError(C.c_size_t(n)), "ZDICT_trainFromBuffer failed"
    d = buf.raw[:n]
    return d[:4] + int(dict_id).to_bytes(4, "little") + d[8:]       # the Dictionary_ID field (dictionary.cairo:50)


def compress(cctx, orig, d, level, checksum=False, id_flag=True):
    def ok(r):
        assert not L.ZSTD_isError(C.c_size_t(r)), r
    ok(L.ZSTD_CCtx_reset(cctx, C.c_int(ZSTD_reset_session_and_parameters)))
    ok(L.ZSTD_CCtx_setParameter(cctx, C.c_int(ZSTD_c_compressionLevel), C.c_int(level)))
    ok(L.ZSTD_CCtx_setParameter(cctx, C.c_int(ZSTD_c_checksumFlag), C.c_int(int(checksum))))
    ok(L.ZSTD_CCtx_setParameter(cctx, C.c_int(ZSTD_c_dictIDFlag), C.c_int(int(id_flag))))
    if d is not None:
        ok(L.ZSTD_CCtx_loadDictionary(cctx, d, C.c_size_t(len(d))))
    cap = L.ZSTD_compressBound(C.c_size_t(len(orig)))
    cbuf = C.create_string_buffer(cap)
    m = L.ZSTD_compress2(cctx, cbuf, C.c_size_t(cap), orig, C.c_size_t(len(orig)))
    ok(m)
    return cbuf.raw[:m]


def header_id(z):
    """(Dictionary_ID, width of its field) of a frame header (frame.cairo:207-225)."""
    d = z[4]
    at = 5 + (0 if d & 0x20 else 1)
    w = (0, 1, 2, 4)[d & 3]
    return int.from_bytes(z[at:at + w], "little"), w


def raw_frame_with_id(data, dict_id):
    """One frame of Raw blocks whose header names `dict_id` in a 4-byte field (no content size, window 2^17)."""
    out = bytearray(b"\x28\xb5\x2f\xfd" + bytes([0x03, 0x38]) + int(dict_id).to_bytes(4, "little"))
    chunks = [data[i:i + 65536] for i in range(0, len(data), 65536)]
    for k, c in enumerate(chunks):
        v = (1 if k == len(chunks) - 1 else 0) | (len(c) << 3)
        out += bytes([v & 255, (v >> 8) & 255, (v >> 16) & 255]) + c
    return bytes(out)


def main():
    os.makedirs(OUT, exist_ok=True)
    for n in os.listdir(OUT):
        os.remove(os.path.join(OUT, n))
    rng = np.random.default_rng(20261015)
    dicts = {k: train(fam, rng, did) for k, (fam, did) in DICTS.items()}
    for k, d in dicts.items():
        open(os.path.join(OUT, f"dict_{k}.bin"), "wb").write(d)
    cctx, dctx = C.c_void_p(L.ZSTD_createCCtx()), C.c_void_p(L.ZSTD_createDCtx())
    frames = []        # (name, dictionary key or None, original, frame)

    def add(name, key, orig, level, checksum=False, id_flag=True):
        z = compress(cctx, orig, dicts[key] if key else None, level, checksum, id_flag)
        d = dicts[key] if key else None
        back = C.create_string_buffer(len(orig) + 1)
        r = L.ZSTD_decompress_usingDict(dctx, back, C.c_size_t(len(orig) + 1), z, C.c_size_t(len(z)), d, C.c_size_t(len(d) if d else 0))
        assert r == len(orig) and back.raw[:r] == orig, name
        frames.append((name, key, orig, z))

    for key in "abcdx":
        fam = DICTS[key][0]
        for k in range(3):                                              # small records: the first block leans on the dictionary
            add(f"{key}_small_{k}", key, record(fam, rng, 1000 + k), 3, checksum=k == 1)
        if key == "x":
            continue
        for k, level in enumerate((3, 19)):                             # several KB
            add(f"{key}_multi_l{level}", key, b"".join(record(fam, rng, 2000 + 50 * k + j) for j in range(40)), level, checksum=level == 19)
        big, j = b"", 0
        while len(big) <= 140 * 1024:                                   # > 128 KiB: two blocks
            big += record(fam, rng, 3000 + j); j += 1
        add(f"{key}_big", key, big, 3, checksum=True)
        add(f"{key}_noid", key, record(fam, rng, 4000), 3, id_flag=False)   # no Dictionary_ID field: for no_id_dict
    for k, fam in enumerate(("users", "sensors")):                      # plain frames, no dictionary
        add(f"plain_{k}", None, b"".join(record(fam, rng, 5000 + j) for j in range(12)), 3, checksum=k == 1)
    raw_orig = b"".join(record("chat", rng, 6000 + j) for j in range(6))
    frames.append(("x_raw", "x", raw_orig, raw_frame_with_id(raw_orig, DICTS["x"][1])))

    manifest = {"dictionaries": {}, "frames": {}}
    for k, d in dicts.items():
        manifest["dictionaries"][f"dict_{k}"] = {"file": f"dict_{k}.bin", "id": DICTS[k][1], "family": DICTS[k][0],
                                                   "registered": k != "x", "sha256": hashlib.sha256(d).hexdigest()}
    for name, key, orig, z in frames:
        did, width = header_id(z)
        open(os.path.join(OUT, name + ".zst"), "wb").write(z)
        small = len(orig) <= ORIG_MAX
        if small:
            open(os.path.join(OUT, name + ".orig"), "wb").write(orig)
        manifest["frames"][name] = {"dictionary": f"dict_{key}" if key else None, "id": did, "id_width": width,
                                    "has_checksum": bool(z[4] & 4), "orig_len": len(orig), "orig_sha256": hashlib.sha256(orig).hexdigest(),
                                    "orig_committed": small, "zst_len": len(z)}
        print(f"{name}: {len(orig)} -> {len(z)} bytes, Dictionary_ID {did:#x} in {width} bytes")
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    total = sum(os.path.getsize(os.path.join(OUT, n)) for n in os.listdir(OUT))
    print(f"{len(frames)} frames, {total} bytes in {OUT}")


if __name__ == "__main__":
    main()
