/*
 * TEST INFRASTRUCTURE ONLY — runs cz_compress_frames_kernel (the unmodified czstd_enc.hip) on the CPU through
 * tests/emu/hip/hip_runtime.h, under ASan+UBSan: one workgroup of 256 lanes (four waves) at a time, a grid of two.
 * usage: emu_encode <batch.bin> <result.bin>
 *   batch.bin : u64 n, u32 flags, then n x { u64 in_len, u64 out_cap, in bytes }
 *   result.bin: n x { cz_compress_result, the whole output region (out_cap bytes; 0xEE where nothing was written) }
 * Inputs sit one byte past the start of an exact-size heap block (unaligned), outputs in another exact-size block.
 */
#define EMU_ENCODE
#include "emu_harness.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    emu_batch b;
    if (fread(&b.n, 8, 1, f) != 1 || fread(&b.flags, 4, 1, f) != 1 || !emu_read_batch(f, &b)) return 2;
    const int grid = 2;
    uint8_t* scratch = (uint8_t*)malloc((size_t)grid * CZE_SCRATCH_BYTES);
    const cz_enc_args a = emu_enc_args(b, scratch, CZE_SCRATCH_BYTES);
    emu_launch(grid, CZE_THREADS, [&] { cz_compress_frames_kernel(a); });
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    emu_write_results(g, &b);
    free(scratch);
    return 0;
}
