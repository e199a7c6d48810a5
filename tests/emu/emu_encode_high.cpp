/*
 * TEST INFRASTRUCTURE ONLY — runs CZ_COMPRESS_HIGH (the unmodified czstd_enc.hip, czstd_encsplit.hip, czstd_encfse.hip and
 * czstd_enchigh.hip) on the CPU through tests/emu/hip/hip_runtime.h, under ASan+UBSan: one workgroup of 256 lanes (four waves) at
 * a time, a grid of two.  The batch's flags pick the kernel as the host library does:
 *     HIGH / HIGH | CHECKSUM                cz_compress_frames_high_kernel
 *     FSE_TABLES / FSE_TABLES | CHECKSUM    cz_compress_frames_fse_kernel, for the comparisons
 * Workgroups run one after another, so this checks the format and the bookkeeping, not concurrency.  Every scratch block has its
 * exact size.
 * usage: emu_encode_high <batch.bin> <result.bin>
 *   batch.bin : u64 n, u32 flags, then n x { u64 in_len, u64 out_cap, in bytes }
 *   result.bin: n x { cz_compress_result, the whole output region (out_cap bytes; 0xEE where nothing was written) }
 * Inputs sit one byte past the start of an exact-size heap block (unaligned), outputs in another exact-size block.
 */
#define EMU_ENCODE
#include "emu_harness.h"
#include "czstd_encsplit.hip"
#include "czstd_encfse.hip"
#include "czstd_enchigh.hip"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    emu_batch b;
    if (fread(&b.n, 8, 1, f) != 1 || fread(&b.flags, 4, 1, f) != 1 || !emu_read_batch(f, &b)) return 2;
    const bool high = b.flags & CZ_COMPRESS_HIGH;
    if (b.flags & ~(CZ_COMPRESS_CHECKSUM | CZ_COMPRESS_HIGH | CZ_COMPRESS_FSE_TABLES) || high == !!(b.flags & CZ_COMPRESS_FSE_TABLES)) return 2;
    const int grid = 2;
    const size_t stride = high ? CZE_HIGH_SCRATCH_BYTES : CZE_FSE_SCRATCH_BYTES;
    uint8_t* scratch = (uint8_t*)malloc((size_t)grid * stride);
    const cz_enc_args a = emu_enc_args(b, scratch, stride);
    if (b.n) emu_launch(grid, CZE_THREADS, [&] {
        if (high) cz_compress_frames_high_kernel(a);
        else cz_compress_frames_fse_kernel(a);
    });
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    emu_write_results(g, &b);
    free(scratch);
    return 0;
}
