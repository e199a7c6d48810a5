"""Small records of the four families of tests/golden/multidict (the record() generator of scripts/gen_multidict_vectors.py,
restated so that the tests need nothing outside tests/), their dictionaries, and libzstd's dictionary compressor when the host
has it.  Test infrastructure only."""
import ctypes

import numpy as np

import multidict_data as md

FAMILIES = (("users", "dict_a"), ("access_log", "dict_b"), ("sensors", "dict_c"), ("orders", "dict_d"))


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
    raise ValueError(family)


def records(per_family=200, seed=7):
    """[(family index, record)]: per_family records of each family, families interleaved."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(per_family):
        for j, (fam, _) in enumerate(FAMILIES):
            out.append((j, record(fam, rng, i)))
    return out


def dictionaries():
    """The four raw dictionaries, in family order."""
    return [md.dict_bytes(name) for _, name in FAMILIES]


_z = None


def libzstd():
    """libzstd.so.1 with the calls these tests use, or None."""
    global _z
    if _z is None:
        try:
            z = ctypes.CDLL("libzstd.so.1")
            for name, res, args in (("ZSTD_compress_usingDict", ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                                               ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]),
                                    ("ZSTD_decompress_usingDict", ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                                                 ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]),
                                    ("ZSTD_createCCtx", ctypes.c_void_p, []), ("ZSTD_createDCtx", ctypes.c_void_p, []),
                                    ("ZSTD_isError", ctypes.c_uint, [ctypes.c_size_t]), ("ZSTD_compressBound", ctypes.c_size_t, [ctypes.c_size_t])):
                fn = getattr(z, name)
                fn.restype, fn.argtypes = res, args
            _z = (z, z.ZSTD_createCCtx(), z.ZSTD_createDCtx())
        except (OSError, AttributeError):
            _z = False
    return _z or None


def zstd_compress_dict(data, dictionary, level=1):
    z, cctx, _ = libzstd()
    cap = z.ZSTD_compressBound(len(data))
    out = ctypes.create_string_buffer(cap)
    r = z.ZSTD_compress_usingDict(cctx, out, cap, bytes(data), len(data), bytes(dictionary), len(dictionary), level)
    assert not z.ZSTD_isError(r)
    return out.raw[:r]


def zstd_decompress_dict(frame, n, dictionary):
    """libzstd's decode of `frame` with `dictionary` (None: no dictionary), or None when it fails."""
    z, _, dctx = libzstd()
    out = ctypes.create_string_buffer(n + 1)
    d = bytes(dictionary) if dictionary is not None else None
    r = z.ZSTD_decompress_usingDict(dctx, out, n + 1, bytes(frame), len(frame), d, len(d) if d else 0)
    return None if z.ZSTD_isError(r) else out.raw[:r]


def manifest_batch():
    """(buffers, dict_index) of the sha256 manifest tests/golden/compress_dict/manifest.json (scripts/gen_compress_dict_manifest.py):
    records of the four families with their dictionaries, then the special inputs of compress_frames without a dictionary and
    with the first one."""
    import compress_frames as cf
    recs = records(25, seed=99)
    sp = [b for _, b in sorted(cf.special_inputs().items())]
    bufs = [b for _, b in recs] + sp + sp
    idx = [j for j, _ in recs] + [0xFFFFFFFF] * len(sp) + [0] * len(sp)
    return bufs, idx
