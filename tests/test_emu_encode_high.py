"""CZ_COMPRESS_HIGH (cz_compress_frames_high_kernel; czstd_enc.hip, czstd_encfse.hip and czstd_enchigh.hip unmodified) on the CPU SIMT
emulator under ASan + UBSan (tests/emu/emu_encode_high.cpp).  Every frame must decode to its input under the oracle (status 0,
every byte consumed) and under libzstd where the host has it, stay within cz_compress_bound and leave 0xEE past bytes_written.
The inputs and what their frames must look like come from tests/compress_high.py, which shares no code with the kernel.  Inputs
stay at or below 60 000 bytes but for the two-block one (140 000) and the one whose first block is Raw, which cannot be smaller
than a block.  No GPU needed."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import compress_edges as ce
import compress_frames as cf
import compress_high as ch
import emu_encode_high_runner as emu
import oracle
from compress_split import blocks_of

pytestmark = pytest.mark.xdist_group(name="emu_encode_high")
BLOCK = 128 << 10
TOO_SMALL = 900
H, F = emu.HIGH, emu.FSE_TABLES


def check(name, b, r, region, flags):
    assert int(r["status"]) == 0, name
    n = int(r["bytes_written"])
    frame = region[:n]
    assert n <= emu.compress_bound(len(b)) == len(region), (name, n)
    assert set(region[n:]) <= {0xEE}, f"{name}: bytes past bytes_written were touched"
    assert int(r["bytes_read"]) == len(b) and int(r["blocks"]) == max(1, -(-len(b) // BLOCK)), name
    assert int(r["flags"]) == flags, (name, int(r["flags"]))
    st, out, info = oracle.decode_frame(frame, cap=len(b) + 64)
    assert st == 0 and out == b and info["consumed"] == n, (name, st)
    assert info["content_size"] == len(b)
    if flags & emu.CHECKSUM:
        assert info["has_checksum"] and info["checksum"] == oracle.xxh64(b) & 0xFFFFFFFF == int(r["checksum"]), name
    if cf.libzstd():
        assert cf.libzstd_decompress(frame, len(b)) == b, f"{name}: libzstd"
    return frame


@pytest.fixture(scope="module")
def built():
    return dict(ch.constructed(), two_blocks=(ch.two_blocks(), ch.expect_two_blocks),
                raw_then_compressed=(ch.raw_then_compressed(), ch.expect_raw_then_compressed))


class Runs:
    """The emulator runs of this file, name -> (inputs, flags, results), each made when a test first asks for it: the test workers
    share no fixtures, so a worker runs only what its own tests need.  need() runs what is missing two at a time (each run is one
    mostly serial program)."""

    def __init__(self, jobs, late):
        self.jobs, self.late, self.got = jobs, late, {}

    def need(self, *keys):
        missing = [k for k in keys if k not in self.got and k in self.jobs]
        with ThreadPoolExecutor(2) as ex:
            fut = {k: ex.submit(emu.run, self.jobs[k][0], flags=self.jobs[k][1]) for k in missing}
            for k, f in fut.items():
                self.got[k] = (self.jobs[k][0], self.jobs[k][1], f.result())
        for k in keys:
            if k not in self.got:
                self.got[k] = self.late[k](self)
        return self

    def __getitem__(self, key):
        return self.need(key).got[key]


@pytest.fixture(scope="module")
def runs(built):
    corpus = [b for _, b in cf.corpus_originals(max_len=6000)]
    special = list(cf.special_inputs().values())
    one = [built[k][0].data for k in ch.constructed()]
    two, raw1 = built["two_blocks"][0].data, built["raw_then_compressed"][0].data
    jobs = {
        "corpus_high": (corpus, H), "corpus_fse": (corpus, F),
        "constructed": (one, H), "lazy_fse": ([one[4]], F),
        "special_high": (special, H), "special_fse": (special, F),
        "two_blocks": ([two, one[2]], H), "raw_first": ([raw1], H),
        "again_1": ([one[5], b"", one[2], one[3]], H), "again_2": ([one[2], one[3], one[5]], H | emu.CHECKSUM),
    }

    def cap_minus_1(r):                                                 # the full two-block frame: one byte short of it
        need = int(r["two_blocks"][2][0][0]["bytes_written"])
        return ([two, one[2]], H, emu.run([two, one[2]], caps=[need - 1, emu.compress_bound(len(one[2]))], flags=H))
    emu.build()
    return Runs(jobs, {"cap_minus_1": cap_minus_1})


def frames(runs, key):
    bufs, flags, res = runs[key]
    return [check(f"{key}[{i}]", b, r, region, flags) for i, (b, (r, region)) in enumerate(zip(bufs, res))]


def test_small_corpus_originals(runs):
    """The 45 originals of at most 6 000 bytes: the total at this level is strictly below the CZ_COMPRESS_FSE_TABLES total of the same
    emulator.  No bound per file: a lazy parse may lose a few bytes on one."""
    runs.need("corpus_high", "corpus_fse")
    high, fse = frames(runs, "corpus_high"), frames(runs, "corpus_fse")
    assert len(high) == 45
    total_high, total_fse = sum(map(len, high)), sum(map(len, fse))
    print(f"small corpus originals: {total_high} bytes with CZ_COMPRESS_HIGH, {total_fse} with CZ_COMPRESS_FSE_TABLES")
    assert total_high < total_fse


@pytest.mark.parametrize("name", list(ch.constructed()))
def test_constructed(runs, built, name):
    b, expect = built[name]
    frame = frames(runs, "constructed")[list(ch.constructed()).index(name)]
    expect(ce.analyse(frame, b.data), b)


def test_lazy_sites_without_the_level(runs, built):
    """The CZ_COMPRESS_FSE_TABLES frame of the same input takes the short match at every site."""
    b, _ = built["lazy_sites"]
    (frame,) = frames(runs, "lazy_fse")
    ch.expect_lazy_sites(ce.analyse(frame, b.data), b, high=False)


def test_special_inputs(runs):
    runs.need("special_high", "special_fse")
    high, fse = frames(runs, "special_high"), frames(runs, "special_fse")
    names = list(cf.special_inputs())
    for k in ("empty", "one", "three", "rle64k", "random64k"):          # no sequences: byte for byte the FSE_TABLES frame
        assert high[names.index(k)] == fse[names.index(k)], k


def test_two_blocks(runs, built):
    b, expect = built["two_blocks"]
    frame = frames(runs, "two_blocks")[0]
    expect(ce.analyse(frame, b.data), b)


def test_raw_block_leaves_no_history(runs, built):
    b, expect = built["raw_then_compressed"]
    (frame,) = frames(runs, "raw_first")
    expect(ce.analyse(frame, b.data), b)


def test_bytes_do_not_depend_on_the_batch(runs):
    """The same buffers at other positions of batches of other sizes (and with the checksum: only the header bit and the last four
    bytes differ)."""
    runs.need("constructed", "again_1", "again_2", "two_blocks")
    one, a1, a2 = frames(runs, "constructed"), frames(runs, "again_1"), frames(runs, "again_2")
    assert a1 == [one[5], a1[1], one[2], one[3]] and len(a1[1]) == 9
    assert frames(runs, "two_blocks")[1] == one[2]
    for with_sum, plain in zip(a2, (one[2], one[3], one[5])):
        assert with_sum[:4] == plain[:4] and with_sum[4] == plain[4] | 4 and with_sum[5:-4] == plain[5:]


def test_output_too_small_is_a_block_aligned_prefix(runs):
    full, neighbour = frames(runs, "two_blocks")
    runs.need("cap_minus_1")
    hl, blocks = blocks_of(full)
    assert len(blocks) == 2
    (r, region), (rn, regn) = runs.got["cap_minus_1"][2]
    assert int(r["status"]) == TOO_SMALL and int(r["flags"]) == H
    w = int(r["bytes_written"])
    assert w == blocks[1][0] and region[:w] == full[:w]                 # the header and the one whole block that fits
    assert int(r["blocks"]) == 1 and int(r["bytes_read"]) == BLOCK
    assert set(region[w:]) <= {0xEE}
    assert int(rn["status"]) == 0 and regn[:int(rn["bytes_written"])] == neighbour and set(regn[len(neighbour):]) <= {0xEE}
