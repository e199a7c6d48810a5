/*
 * TEST INFRASTRUCTURE ONLY — runs the records level (CZ_COMPRESS_RECORDS: cz_compress_records_kernel and
 * cz_compress_records_dict_kernel, the unmodified czstd_encrec.hip behind czstd_enc.hip, czstd_encsplit.hip, czstd_encfse.hip and
 * czstd_encfast.hip) on the CPU through tests/emu/hip/hip_runtime.h, under ASan+UBSan: each dictionary parsed by
 * cz_dict_setup_kernel and prepared by cz_enc_dict_prep_kernel (a grid of two), then the records kernel, a grid of two workgroups of
 * 256 lanes (four waves, each on records of its own), one workgroup at a time.  Workgroups run one after another, so this checks
 * the format and the bookkeeping, not concurrency.
 * usage: emu_encode_records <batch.bin> <result.bin>
 *   batch.bin : u64 n, u32 flags, u32 k, k x { u64 len, dictionary bytes }, u32 mode (0: cz_compress_records_kernel; 1: the dict
 *               kernel without an index; 2: the dict kernel with one), then n x { u64 in_len, u64 out_cap, u32 dict_index, in bytes }
 *   result.bin: u64 the level's largest record, then n x { cz_compress_result, the whole output region (out_cap bytes; 0xEE where
 *               nothing was written) }
 * Inputs sit one byte past the start of an exact-size heap block (unaligned), outputs in another exact-size block, the scratch in
 * an exact-size block, each dictionary in an exact-size block of its own.
 */
#define EMU_ENCODE
#include "emu_harness.h"
#include "czstd_encsplit.hip"
#include "czstd_encfse.hip"
#include "czstd_encfast.hip"
#include "czstd_encrec.hip"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    emu_batch b; emu_dicts d; uint32_t k, mode;
    if (fread(&b.n, 8, 1, f) != 1 || fread(&b.flags, 4, 1, f) != 1 || fread(&k, 4, 1, f) != 1) return 2;
    if (const int st = emu_load_dicts(f, k, &d)) return st;
    if (fread(&mode, 4, 1, f) != 1 || mode > 2 || !(b.flags & CZ_COMPRESS_RECORDS) || !emu_read_batch(f, &b, true)) return 2;
    const int grid = 2;
    uint8_t* scratch = (uint8_t*)malloc((size_t)grid * CZE_RECORDS_SCRATCH_BYTES);
    const cz_enc_args a = emu_enc_args(b, scratch, CZE_RECORDS_SCRATCH_BYTES);
    cz_enc_dargs dd; memset(&dd, 0, sizeof dd);
    dd.dicts = d.table; dd.dict_index = mode == 2 ? b.dict_index : nullptr; dd.ndicts = k;
    if (b.n) emu_launch(grid, CZE_THREADS, [&] { if (mode) cz_compress_records_dict_kernel(a, dd); else cz_compress_records_kernel(a); });
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    { const uint64_t mx = CZR_MAX; fwrite(&mx, 8, 1, g); }
    emu_write_results(g, &b);
    free(scratch); emu_free_dicts(&d);
    return 0;
}
