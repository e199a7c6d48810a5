/*
 * TEST INFRASTRUCTURE ONLY — runs the CZ_COMPRESS_SPLIT kernels (cz_compress_plan_kernel, then cz_compress_segments_kernel; the
 * unmodified czstd_enc.hip and czstd_encsplit.hip) on the CPU through tests/emu/hip/hip_runtime.h, under ASan+UBSan: one workgroup
 * of 256 lanes (four waves) at a time, a grid of two for the segments.  Built with one-block segments and a small overlap
 * (the Makefile's DEFS).  Workgroups run one after another, so this checks the format and the chain bookkeeping, not concurrency:
 * the first workgroup claims every unit in order and no wait ever polls twice.
 * usage: emu_encode_split <batch.bin> <result.bin>
 *   batch.bin : u64 n, u32 flags, then n x { u64 in_len, u64 out_cap, in bytes }
 *   result.bin: u64 S, u64 W, then n x { cz_compress_result, the whole output region (out_cap bytes; 0xEE where nothing was written) }
 * Inputs sit one byte past the start of an exact-size heap block (unaligned), outputs in another exact-size block.
 */
#define EMU_ENCODE
#include "emu_harness.h"
#include "czstd_encsplit.hip"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    emu_batch b;
    if (fread(&b.n, 8, 1, f) != 1 || fread(&b.flags, 4, 1, f) != 1 || !emu_read_batch(f, &b)) return 2;
    const uint64_t n = b.n;
    const int grid = 2;
    uint8_t* scratch = (uint8_t*)malloc((size_t)grid * CZE_SPLIT_SCRATCH_BYTES);
    unsigned long long counter = 0;
    unsigned long long* plan = (unsigned long long*)malloc((3 * n + 1) * sizeof(unsigned long long));   /* exact size, not cleared */
    memset(plan, 0xA5, (3 * n + 1) * sizeof(unsigned long long));
    cz_encsplit_args sa; memset(&sa, 0, sizeof sa);
    sa.a = emu_enc_args(b, scratch, CZE_SPLIT_SCRATCH_BYTES); sa.a.work_counter = nullptr;   /* (the units come from sa.counter) */
    sa.unit_base = plan; sa.fstate = plan + n + 1; sa.counter = &counter;
    if (n) {                                                            /* the plan kernel (one workgroup), then the segments */
        emu_launch(1, CZE_THREADS, [&] { cz_compress_plan_kernel(sa.a.in_len, sa.a.n, sa.a.flags, sa.unit_base, sa.fstate); });
        emu_launch(grid, CZE_THREADS, [&] { cz_compress_segments_kernel(sa); });
    }
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    { const uint64_t sw[2] = { CZE_SEG, CZE_OVERLAP }; fwrite(sw, 8, 2, g); }
    emu_write_results(g, &b);
    free(plan); free(scratch);
    return 0;
}
