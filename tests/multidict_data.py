"""The several-dictionaries fixtures of tests/golden/multidict (scripts/gen_multidict_vectors.py): dictionaries, frames and
their originals.  Originals that are not committed (the frames over 128 KiB) are checked by the manifest's sha256."""
import hashlib
import json
import os

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multidict")
MANIFEST = json.load(open(os.path.join(DIR, "manifest.json")))
REGISTERED = ("dict_a", "dict_b", "dict_c", "dict_d")
UNREGISTERED = "dict_x"
UNKNOWN_ID = MANIFEST["dictionaries"][UNREGISTERED]["id"]


def dict_path(name):
    return os.path.join(DIR, MANIFEST["dictionaries"][name]["file"])


def dict_bytes(name):
    return open(dict_path(name), "rb").read()


class Frame:
    def __init__(self, name):
        m = MANIFEST["frames"][name]
        self.name, self.meta = name, m
        self.zst = open(os.path.join(DIR, name + ".zst"), "rb").read()
        self.orig = open(os.path.join(DIR, name + ".orig"), "rb").read() if m["orig_committed"] else None
        self.dictionary, self.id, self.orig_len = m["dictionary"], m["id"], m["orig_len"]

    def matches(self, out: bytes) -> bool:
        """`out` is the original, byte for byte."""
        if len(out) != self.orig_len:
            return False
        return out == self.orig if self.orig is not None else hashlib.sha256(out).hexdigest() == self.meta["orig_sha256"]

    def __repr__(self):
        return self.name


def frames(pred=lambda f: True):
    out = [Frame(n) for n in sorted(MANIFEST["frames"])]
    return [f for f in out if pred(f)]


def registered_frames():
    """Frames whose header names one of the four registered dictionaries."""
    return frames(lambda f: f.dictionary in REGISTERED and f.id != 0)


def noid_frames():
    return frames(lambda f: f.dictionary in REGISTERED and f.id == 0)


def plain_frames():
    return frames(lambda f: f.dictionary is None)


def unknown_frames():
    """Frames whose header names the fifth dictionary, which is never registered (x_raw: Raw blocks only)."""
    return frames(lambda f: f.dictionary == UNREGISTERED)
