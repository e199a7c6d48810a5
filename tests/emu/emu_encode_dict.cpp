/*
 * TEST INFRASTRUCTURE ONLY — runs the dictionary compressor (the unmodified czstd_enc.hip and czstd_kernels.hip) on the CPU through
 * tests/emu/hip/hip_runtime.h, under ASan+UBSan: each dictionary parsed by cz_dict_setup_kernel, prepared by cz_enc_dict_prep_kernel
 * (a grid of two), then cz_compress_frames_dict_kernel (a grid of two), one workgroup at a time.
 * usage: emu_encode_dict <batch.bin> <result.bin> [<tables.bin>]
 *   batch.bin : u64 n, u32 flags, u32 k, k x { u64 len, dictionary bytes }, u32 has_index, then n x { u64 in_len, u64 out_cap,
 *               u32 dict_index, in bytes }
 *   result.bin: n x { cz_compress_result, the whole output region (out_cap bytes; 0xEE where nothing was written) }
 *   tables.bin: k x the prepared hash table (CzeDict::htab, 2^14 u32) of each dictionary, as cz_enc_dict_prep_kernel left it
 * Inputs sit one byte past the start of an exact-size heap block (unaligned), outputs in another exact-size block, each dictionary
 * in an exact-size block of its own.
 */
#define EMU_ENCODE
#include "emu_harness.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    emu_batch b; emu_dicts d; uint32_t k, has_index;
    if (fread(&b.n, 8, 1, f) != 1 || fread(&b.flags, 4, 1, f) != 1 || fread(&k, 4, 1, f) != 1) return 2;
    if (const int st = emu_load_dicts(f, k, &d)) return st;
    if (argc > 3) {
        FILE* tf = fopen(argv[3], "wb"); if (!tf) return 2;
        for (uint32_t j = 0; j < k; j++) fwrite(d.table[j].img->htab, 4, 1u << CZE_HASH_LOG, tf);
        fclose(tf);
    }
    if (fread(&has_index, 4, 1, f) != 1 || !emu_read_batch(f, &b, true)) return 2;
    const int grid = 2;
    uint8_t* scratch = (uint8_t*)malloc((size_t)grid * CZE_SCRATCH_BYTES);
    const cz_enc_args a = emu_enc_args(b, scratch, CZE_SCRATCH_BYTES);
    cz_enc_dargs dd; memset(&dd, 0, sizeof dd);
    dd.dicts = d.table; dd.dict_index = has_index ? b.dict_index : nullptr; dd.ndicts = k;
    emu_launch(grid, CZE_THREADS, [&] { cz_compress_frames_dict_kernel(a, dd); });
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    emu_write_results(g, &b);
    free(scratch); emu_free_dicts(&d);
    return 0;
}
