/*
 * TEST INFRASTRUCTURE ONLY — runs dictionary training (the unmodified czstd_train.hip with czstd_kernels.hip, czstd_enc.hip,
 * czstd_encsplit.hip and czstd_encfse.hip in front of it) on the CPU through tests/emu/hip/hip_runtime.h, under ASan+UBSan: the
 * launches of cz_dictionary_train_device in its order, one workgroup at a time, with the grids given below (the dictionary does not
 * depend on them).
 * usage: emu_train <samples.bin> <result.bin>
 *   samples.bin: u64 n, u64 dict_cap, u32 has_params, u32 dict_id, u32 segment_len, u32 reserved[6], then n x { u64 len, u64 stored,
 *                stored bytes } (stored = len, except where the lengths alone are to be refused)
 *   result.bin : i32 status, u32 pieces, u64 dict_len, the whole output region (dict_cap bytes; 0xEE where nothing was written)
 * Every sample sits in an exact-size heap block of its own, as do the output region and every device array.
 */
#include "emu_harness.h"
#include "czstd_kernels.hip"
#include "czstd_enc.hip"
#include "czstd_encsplit.hip"
#include "czstd_encfse.hip"
#include "czstd_train.hip"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    uint64_t n, dict_cap; uint32_t has_params; cz_train_params pr;
    if (fread(&n, 8, 1, f) != 1 || fread(&dict_cap, 8, 1, f) != 1 || fread(&has_params, 4, 1, f) != 1 || fread(&pr, sizeof pr, 1, f) != 1) return 2;
    std::vector<uint64_t> len(n ? n : 1), off(n ? n : 1);
    std::vector<uint8_t*> blocks;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t stored;
        if (fread(&len[i], 8, 1, f) != 1 || fread(&stored, 8, 1, f) != 1) return 2;
        uint8_t* b = (uint8_t*)malloc(stored ? stored : 1); blocks.push_back(b);
        if (stored && fread(b, 1, stored, f) != stored) return 2;
        off[i] = (uint64_t)(uintptr_t)b;                                 /* base = address 0: any layout is a batch */
    }
    fclose(f);
    uint8_t* dict = (uint8_t*)malloc(dict_cap ? dict_cap : 1); memset(dict, 0xEE, dict_cap);
    int status = cz_train_check_params(n, dict_cap, has_params ? &pr : nullptr);
    uint32_t pieces = 0; uint64_t dict_len = 0;
    std::vector<uint32_t> cum(n + 1);
    if (!status) status = cz_train_check_lengths(len.data(), n, cum.data());
    if (!status) {
        if (!has_params) memset(&pr, 0, sizeof pr);
        const uint32_t total = cum[n];
        const cz_train_plan plan = cz_train_make_plan(dict_cap, pr.segment_len, total);
        cz_train_args a; memset(&a, 0, sizeof a);
        uint32_t* d_cum = (uint32_t*)malloc((n + 1) * 4); memcpy(d_cum, cum.data(), (n + 1) * 4);
        a.base = (const uint8_t*)nullptr; a.off = off.data(); a.len = len.data(); a.cum = d_cum; a.n = (uint32_t)n; a.total = total;
        a.seg_len = plan.seg_len; a.segments = plan.segments; a.content_cap = plan.content_cap; a.dict_id = pr.dict_id;
        a.freq = (uint32_t*)calloc(1u << CZT_FREQ_LOG, 4); a.htab = (uint32_t*)calloc(1u << CZE_HASH_LOG, 4);
        a.content = (uint8_t*)malloc(plan.content_cap); memset(a.content, 0xEE, plan.content_cap);
        a.st = (cz_train_state*)calloc(1, sizeof(cz_train_state)); a.st->cursor = plan.content_cap;
        a.dict = dict;
        if (total <= plan.content_cap) emu_launch(3, CZT_THREADS, [&] { cz_train_concat_kernel(a); });
        else {
            emu_launch(3, CZT_THREADS, [&] { cz_train_freq_kernel(a); });
            const unsigned tiles = (plan.max_range + CZT_TILE - 1) / CZT_TILE;
            for (uint32_t r = 0; r < plan.rounds;) {
                for (uint32_t k = 0; k < plan.segments; k++, r++) { emu_launch((int)tiles, CZT_THREADS, [&] { cz_train_score_kernel(a, r); }); emu_launch(1, CZT_THREADS, [&] { cz_train_commit_kernel(a); }); }
                if (a.st->cursor < plan.seg_len) break;
            }
        }
        emu_launch(2, CZT_THREADS, [&] { cz_train_image_kernel(a); });
        emu_launch(3, CZT_THREADS, [&] { cz_train_stats_kernel(a); });
        emu_launch(1, CZT_THREADS, [&] { cz_train_finish_kernel(a); });
        status = (int)a.st->status; pieces = a.st->pieces; dict_len = a.st->dict_len;
        free(d_cum); free(a.freq); free(a.htab); free(a.content); free(a.st);
    }
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    fwrite(&status, 4, 1, g); fwrite(&pieces, 4, 1, g); fwrite(&dict_len, 8, 1, g); fwrite(dict, 1, dict_cap, g);
    fclose(g);
    free(dict);
    for (uint8_t* b : blocks) free(b);
    return 0;
}
