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
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

/* what the encoder needs that hip/hip_runtime.h lacks: atomicMax (32 bits for the hash table, 64 for the chain word) and the
   sleep of a poll loop; the agent-scope loads and stores come from czstd_kernels.hip's CZ_EMU branch */
template <class T> static inline T emu_atomic_max(T* p, T v) {
    T cur = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (cur < v && !__atomic_compare_exchange_n(p, &cur, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return cur;
}
static inline uint32_t atomicMax(uint32_t* p, uint32_t v) { return emu_atomic_max(p, v); }
static inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) { return emu_atomic_max(p, v); }
#define __builtin_amdgcn_s_sleep(x) ((void)sched_yield())
#include <sched.h>

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
#include <unistd.h>
/* watchdog: if no lane passes a barrier for 20 s, the run ends */
static void* emu_watchdog(void*) {
    uint64_t last = 0; int idle = 0;
    for (;;) {
        sleep(1);
        uint64_t sum = 0; for (int i = 0; i < EMU_MAX_THREADS; i++) sum += emu_sync_count[i];
        if (sum != last) { last = sum; idle = 0; continue; }
        if (++idle < 20) continue;
        fprintf(stderr, "EMU HANG\n");
        _exit(3);
    }
    return nullptr;
}

#include "czstd_kernels.hip"
#include "czstd_enc.hip"
#include "czstd_encsplit.hip"
#include "czstd_encfse.hip"
#include "czstd_encfast.hip"

struct lane_arg { cz_enc_args a; unsigned lane, block; };
static void* lane_main(void* p) {
    lane_arg* la = (lane_arg*)p;
    threadIdx.x = la->lane; blockIdx.x = la->block;
    cz_compress_frames_fast_kernel(la->a);
    return nullptr;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    uint64_t n; uint32_t flags;
    if (fread(&n, 8, 1, f) != 1 || fread(&flags, 4, 1, f) != 1) return 2;
    std::vector<uint64_t> in_off(n), in_len(n), out_off(n), out_cap(n);
    std::vector<uint8_t> in(1, 0x5A); uint64_t out_total = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t l, c; if (fread(&l, 8, 1, f) != 1 || fread(&c, 8, 1, f) != 1) return 2;
        in_off[i] = in.size(); in_len[i] = l; out_cap[i] = c; out_off[i] = out_total; out_total += c;
        size_t at = in.size(); in.resize(at + l);
        if (l && fread(in.data() + at, 1, l, f) != l) return 2;
    }
    fclose(f);
    uint8_t* in_exact = (uint8_t*)malloc(in.size()); memcpy(in_exact, in.data(), in.size());
    uint8_t* out = (uint8_t*)malloc(out_total ? out_total : 1); memset(out, 0xEE, out_total);
    cz_compress_result* res = (cz_compress_result*)malloc((n ? n : 1) * sizeof(cz_compress_result));
    memset(res, 0xA5, (n ? n : 1) * sizeof(cz_compress_result));          /* a record nobody writes shows up */
    if ((flags & ~CZ_COMPRESS_CHECKSUM) != CZ_COMPRESS_FAST) return 2;
    const int grid = 2, nthreads = CZE_THREADS;
    const size_t stride = CZE_FAST_SCRATCH_BYTES;
    uint8_t* scratch = (uint8_t*)malloc((size_t)grid * stride);
    uint32_t counter32 = 0;
    cz_enc_args a; memset(&a, 0, sizeof a);
    a.in_base = in_exact; a.in_off = in_off.data(); a.in_len = in_len.data();
    a.out_base = out; a.out_off = out_off.data(); a.out_cap = out_cap.data(); a.results = res;
    a.n = (uint32_t)n; a.flags = flags; a.scratch = scratch; a.scratch_stride = stride; a.work_counter = &counter32;
    { pthread_t wd; pthread_create(&wd, nullptr, emu_watchdog, nullptr); pthread_detach(wd); }
    for (int w = 0; w < EMU_MAX_WAVES; w++) pthread_barrier_init(&emu_wbar[w], nullptr, 64);
    blockDim.x = (unsigned)nthreads; gridDim.x = (unsigned)grid;
    pthread_barrier_init(&emu_barrier, nullptr, (unsigned)nthreads);
    for (int b = 0; n && b < grid; b++) {
        std::vector<pthread_t> th((size_t)nthreads); std::vector<lane_arg> la((size_t)nthreads);
        for (int l = 0; l < nthreads; l++) {
            la[l].a = a; la[l].lane = (unsigned)l; la[l].block = (unsigned)b;
            pthread_create(&th[l], nullptr, lane_main, &la[l]);
        }
        for (int l = 0; l < nthreads; l++) pthread_join(th[l], nullptr);
    }
    pthread_barrier_destroy(&emu_barrier);
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    { const uint64_t sw[2] = { CZQ_SUB, CZQ_GROUP }; fwrite(sw, 8, 2, g); }
    for (uint64_t i = 0; i < n; i++) {
        fwrite(&res[i], sizeof(cz_compress_result), 1, g);
        fwrite(out + out_off[i], 1, out_cap[i], g);
    }
    fclose(g);
    free(scratch); free(res); free(out); free(in_exact);
    return 0;
}
