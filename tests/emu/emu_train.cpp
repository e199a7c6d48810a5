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
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

/* what the kernels need that hip/hip_runtime.h lacks: atomicMax, 32 bits for the hash table and 64 for the best window (and the
   sleep of czstd_encsplit.hip's poll loops, which are compiled but never run here) */
#define __builtin_amdgcn_s_sleep(x) ((void)sched_yield())
template <class T> static inline T emu_atomic_max(T* p, T v) {
    T cur = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (cur < v && !__atomic_compare_exchange_n(p, &cur, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return cur;
}
static inline uint32_t atomicMax(uint32_t* p, uint32_t v) { return emu_atomic_max(p, v); }
static inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) { return emu_atomic_max(p, v); }

thread_local emu_dim3 threadIdx;
thread_local emu_dim3 blockIdx;
emu_dim3 gridDim;
emu_dim3 blockDim;
pthread_barrier_t emu_barrier;
pthread_barrier_t emu_wbar[EMU_MAX_WAVES];
volatile uint64_t emu_xchg_all[EMU_MAX_WAVES][64];
void* volatile emu_site[EMU_MAX_THREADS];
void* volatile emu_ring[EMU_MAX_THREADS][64];
volatile uint64_t emu_sync_count[EMU_MAX_THREADS];

#include "czstd_kernels.hip"
#include "czstd_enc.hip"
#include "czstd_encsplit.hip"
#include "czstd_encfse.hip"
#include "czstd_train.hip"

enum { K_FREQ, K_SCORE, K_COMMIT, K_CONCAT, K_IMAGE, K_STATS, K_FINISH };
struct lane_arg { int which; unsigned lane, nblocks; cz_train_args a; uint32_t round; };
/* one thread per lane for the whole launch: the workgroups run one after the other, a barrier between them */
static void* lane_main(void* p) {
    lane_arg* la = (lane_arg*)p;
    threadIdx.x = la->lane;
    for (unsigned b = 0; b < la->nblocks; b++) {
        blockIdx.x = b;
        switch (la->which) {
            case K_FREQ: cz_train_freq_kernel(la->a); break;
            case K_SCORE: cz_train_score_kernel(la->a, la->round); break;
            case K_COMMIT: cz_train_commit_kernel(la->a); break;
            case K_CONCAT: cz_train_concat_kernel(la->a); break;
            case K_IMAGE: cz_train_image_kernel(la->a); break;
            case K_STATS: cz_train_stats_kernel(la->a); break;
            default: cz_train_finish_kernel(la->a); break;
        }
        pthread_barrier_wait(&emu_barrier);
    }
    return nullptr;
}
static void launch(int which, const cz_train_args& a, unsigned nblocks, uint32_t round = 0) {
    blockDim.x = CZT_THREADS; gridDim.x = nblocks;
    pthread_barrier_init(&emu_barrier, nullptr, CZT_THREADS);
    std::vector<pthread_t> th(CZT_THREADS); std::vector<lane_arg> la(CZT_THREADS);
    for (unsigned l = 0; l < CZT_THREADS; l++) {
        la[l].which = which; la[l].lane = l; la[l].nblocks = nblocks; la[l].a = a; la[l].round = round;
        pthread_create(&th[l], nullptr, lane_main, &la[l]);
    }
    for (unsigned l = 0; l < CZT_THREADS; l++) pthread_join(th[l], nullptr);
    pthread_barrier_destroy(&emu_barrier);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    uint64_t n, dict_cap; uint32_t has_params; cz_train_params pr;
    if (fread(&n, 8, 1, f) != 1 || fread(&dict_cap, 8, 1, f) != 1 || fread(&has_params, 4, 1, f) != 1 || fread(&pr, sizeof pr, 1, f) != 1) return 2;
    for (int w = 0; w < EMU_MAX_WAVES; w++) pthread_barrier_init(&emu_wbar[w], nullptr, 64);
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
        if (total <= plan.content_cap) launch(K_CONCAT, a, 3);
        else {
            launch(K_FREQ, a, 3);
            const unsigned tiles = (plan.max_range + CZT_TILE - 1) / CZT_TILE;
            for (uint32_t r = 0; r < plan.rounds;) {
                for (uint32_t k = 0; k < plan.segments; k++, r++) { launch(K_SCORE, a, tiles, r); launch(K_COMMIT, a, 1); }
                if (a.st->cursor < plan.seg_len) break;
            }
        }
        launch(K_IMAGE, a, 2);
        launch(K_STATS, a, 3);
        launch(K_FINISH, a, 1);
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
