/*
 * TEST INFRASTRUCTURE ONLY — runs the fast compression level (CZ_COMPRESS_FAST: cz_compress_frames_fast_kernel, the unmodified
 * czstd_encfast.hip behind czstd_enc.hip, czstd_encsplit.hip and czstd_encfse.hip) on the CPU through tests/emu/hip/hip_runtime.h,
 * under ASan+UBSan: one workgroup of 256 lanes (four waves, each on a sub-block of its own) at a time, a grid of two.  Workgroups
 * run one after another, so this checks the format and the bookkeeping, not concurrency.  The scratch block has its exact size.
 * usage: emu_encode_fast <batch.bin> <result.bin>
 *   batch.bin : u64 n, u32 flags (CZ_COMPRESS_FAST, with or without CZ_COMPRESS_CHECKSUM), then n x { u64 in_len, u64 out_cap, in bytes }
 *   result.bin: u64 sub-block, u64 group, then n x { cz_compress_result, the whole output region (out_cap bytes; 0xEE where nothing
 *               was written) }
 * Inputs sit one byte past the start of an exact-size heap block (unaligned), outputs in another exact-size block.
 */
#define EMU_ENCODE
#include "emu_harness.h"
#include "czstd_encsplit.hip"
#include "czstd_encfse.hip"
#include "czstd_encfast.hip"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    emu_batch b;
    if (fread(&b.n, 8, 1, f) != 1 || fread(&b.flags, 4, 1, f) != 1 || !emu_read_batch(f, &b)) return 2;
    if ((b.flags & ~CZ_COMPRESS_CHECKSUM) != CZ_COMPRESS_FAST) return 2;
    const int grid = 2;
    uint8_t* scratch = (uint8_t*)malloc((size_t)grid * CZE_FAST_SCRATCH_BYTES);
    const cz_enc_args a = emu_enc_args(b, scratch, CZE_FAST_SCRATCH_BYTES);
    if (b.n) emu_launch(grid, CZE_THREADS, [&] { cz_compress_frames_fast_kernel(a); });
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    { const uint64_t sw[2] = { CZQ_SUB, CZQ_GROUP }; fwrite(sw, 8, 2, g); }
    emu_write_results(g, &b);
    free(scratch);
    return 0;
}
