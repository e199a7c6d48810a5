/*
 * TEST INFRASTRUCTURE ONLY — runs CZ_COMPRESS_HIGH_SPLIT (the unmodified czstd_enc.hip, czstd_encsplit.hip, czstd_encfse.hip,
 * czstd_enchigh.hip and czstd_enchighsplit.hip) on the CPU through tests/emu/hip/hip_runtime.h, under ASan+UBSan: one workgroup of
 * 256 lanes (four waves) at a time, a grid of two.  The batch's flags pick the kernel as the host library does:
 *     HIGH_SPLIT / HIGH_SPLIT | CHECKSUM                    cz_compress_plan_kernel, cz_compress_segments_high_kernel
 *     HIGH / HIGH | CHECKSUM                                cz_compress_frames_high_kernel, for the comparisons
 *     SPLIT | FSE_TABLES / SPLIT | FSE_TABLES | CHECKSUM    cz_compress_plan_kernel, cz_compress_segments_fse_kernel, for the comparisons
 * Built with one-block segments and an 8 KiB overlap (high_split.mk).  Workgroups run one after another, so this checks the format
 * and the bookkeeping, not concurrency.  Every scratch, plan and output block has its exact size; the plan starts as 0xA5, the
 * outputs as 0xEE.
 * usage: emu_encode_high_split <batch.bin> <result.bin>
 *   batch.bin : u64 n, u32 flags, then n x { u64 in_len, u64 out_cap, in bytes }
 *   result.bin: u64 S, u64 W, then n x { cz_compress_result, the whole output region (out_cap bytes; 0xEE where nothing was written) }
 * Inputs sit one byte past the start of an exact-size heap block (unaligned), outputs in another exact-size block.
 */
#define EMU_ENCODE
#include "emu_harness.h"
#include "czstd_encsplit.hip"
#include "czstd_encfse.hip"
#include "czstd_enchigh.hip"
#include "czstd_enchighsplit.hip"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    emu_batch b;
    if (fread(&b.n, 8, 1, f) != 1 || fread(&b.flags, 4, 1, f) != 1 || !emu_read_batch(f, &b)) return 2;
    const uint64_t n = b.n;
    const uint32_t level = b.flags & ~CZ_COMPRESS_CHECKSUM;
    const bool hsplit = level == CZ_COMPRESS_HIGH_SPLIT, high = level == CZ_COMPRESS_HIGH;
    if (!hsplit && !high && level != (CZ_COMPRESS_SPLIT | CZ_COMPRESS_FSE_TABLES)) return 2;
    const int grid = 2;
    const size_t stride = high ? CZE_HIGH_SCRATCH_BYTES : CZE_FSE_SPLIT_SCRATCH_BYTES;
    uint8_t* scratch = (uint8_t*)malloc((size_t)grid * stride);
    unsigned long long counter = 0;
    unsigned long long* plan = (unsigned long long*)malloc((3 * n + 1) * sizeof(unsigned long long));   /* exact size, not cleared */
    memset(plan, 0xA5, (3 * n + 1) * sizeof(unsigned long long));
    cz_encsplit_args sa; memset(&sa, 0, sizeof sa);
    sa.a = emu_enc_args(b, scratch, stride);
    sa.unit_base = plan; sa.fstate = plan + n + 1; sa.counter = &counter;
    if (n && !high) emu_launch(1, CZE_THREADS, [&] { cz_compress_plan_kernel(sa.a.in_len, sa.a.n, sa.a.flags, sa.unit_base, sa.fstate); });
    if (n) emu_launch(grid, CZE_THREADS, [&] {
        if (hsplit) cz_compress_segments_high_kernel(sa);
        else if (high) cz_compress_frames_high_kernel(sa.a);
        else cz_compress_segments_fse_kernel(sa);
    });
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    { const uint64_t sw[2] = { CZE_SEG, CZE_OVERLAP }; fwrite(sw, 8, 2, g); }
    emu_write_results(g, &b);
    free(plan); free(scratch);
    return 0;
}
