/*
 * TEST INFRASTRUCTURE ONLY — runs the CZ_COMPRESS_FAST_SPLIT kernels (cz_compress_fast_plan_kernel, then
 * cz_compress_groups_fast_kernel; the unmodified czstd_encfastsplit.hip behind czstd_encfast.hip) on the CPU through
 * tests/emu/hip/hip_runtime.h, under ASan+UBSan: one workgroup of 256 lanes (four waves, each on a sub-block of its own) at a time,
 * a grid of two for the groups.  Workgroups run one after another, so this checks the format and the chain bookkeeping, not
 * concurrency: the first workgroup claims every unit in order and no wait ever polls twice.  The plan and the scratch are heap
 * blocks of their exact size; the plan starts as 0xA5, so a word the plan kernel does not clear shows up.
 * usage: emu_encode_fast_split <batch.bin> <result.bin>
 *   batch.bin : u64 n, u32 flags (CZ_COMPRESS_FAST_SPLIT, with or without CZ_COMPRESS_CHECKSUM), then n x { u64 in_len, u64 out_cap, in bytes }
 *   result.bin: u64 sub-block, u64 group, then n x { cz_compress_result, the whole output region (out_cap bytes; 0xEE where nothing
 *               was written) }
 * Inputs sit one byte past the start of an exact-size heap block (unaligned), outputs in another exact-size block.
 */
#define EMU_ENCODE
#include "emu_harness.h"
#include "czstd_encsplit.hip"
#include "czstd_encfse.hip"
#include "czstd_encfast.hip"
#include "czstd_encfastsplit.hip"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    emu_batch b;
    if (fread(&b.n, 8, 1, f) != 1 || fread(&b.flags, 4, 1, f) != 1 || !emu_read_batch(f, &b)) return 2;
    if ((b.flags & ~CZ_COMPRESS_CHECKSUM) != CZ_COMPRESS_FAST_SPLIT) return 2;
    const uint64_t n = b.n;
    const int grid = 2;
    uint8_t* scratch = (uint8_t*)malloc((size_t)grid * CZE_FAST_SCRATCH_BYTES);
    unsigned long long counter = 0;
    const size_t words = (CZG_FSTATE_WORDS + 1) * n + 1;                /* unit_base, then the per-frame state: exact size, not cleared */
    unsigned long long* plan = (unsigned long long*)malloc(words * sizeof(unsigned long long));
    memset(plan, 0xA5, words * sizeof(unsigned long long));
    cz_encsplit_args sa; memset(&sa, 0, sizeof sa);
    sa.a = emu_enc_args(b, scratch, CZE_FAST_SCRATCH_BYTES); sa.a.work_counter = nullptr;   /* (the units come from sa.counter) */
    sa.unit_base = plan; sa.fstate = plan + n + 1; sa.counter = &counter;
    if (n) {                                                            /* the plan kernel (one workgroup), then the groups */
        emu_launch(1, CZE_THREADS, [&] { cz_compress_fast_plan_kernel(sa.a.in_len, sa.a.n, sa.a.flags, sa.unit_base, sa.fstate); });
        emu_launch(grid, CZE_THREADS, [&] { cz_compress_groups_fast_kernel(sa); });
    }
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    { const uint64_t sw[2] = { CZQ_SUB, CZQ_GROUP }; fwrite(sw, 8, 2, g); }
    emu_write_results(g, &b);
    free(plan); free(scratch);
    return 0;
}
