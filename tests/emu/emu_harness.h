/*
 * TEST INFRASTRUCTURE ONLY — what every emulator driver needs around the unmodified kernel sources: the globals that
 * hip/hip_runtime.h declares, the few device functions it lacks, the watchdog, and emu_launch.  A driver includes this once, ahead
 * of the kernel sources.  With EMU_ENCODE defined first it also includes czstd_kernels.hip and czstd_enc.hip and gives the encode
 * drivers their batch reader, result writer and dictionary set-up; the driver includes the kernel sources of its level after it.
 *
 * The allocation discipline is what makes ASan useful: every array a kernel sees is a heap block of its exact size, the inputs sit
 * one byte past the start of theirs (unaligned), output regions start as 0xEE and result records as 0xA5.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <errno.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>
#include <vector>

/* what the kernels need that hip/hip_runtime.h lacks: atomicMax (32 bits for the hash tables, 64 for the chain word and the
   trainer's best window) and the sleep of a poll loop; the agent-scope loads and stores come from czstd_kernels.hip's CZ_EMU branch */
template <class T> static inline T emu_atomic_max(T* p, T v) {
    T cur = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (cur < v && !__atomic_compare_exchange_n(p, &cur, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return cur;
}
static inline uint32_t atomicMax(uint32_t* p, uint32_t v) { return emu_atomic_max(p, v); }
static inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) { return emu_atomic_max(p, v); }
#define __builtin_amdgcn_s_sleep(x) ((void)sched_yield())

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
static volatile int emu_lane_done[EMU_MAX_THREADS];
static volatile int emu_nthreads = 64;

/* watchdog: if no lane passes a barrier for 20 s, print where every lane waits and end the run */
static void* emu_watchdog(void*) {
    uint64_t last = 0; int idle = 0;
    for (;;) {
        sleep(1);
        uint64_t sum = 0; for (int i = 0; i < EMU_MAX_THREADS; i++) sum += emu_sync_count[i];
        if (sum != last) { last = sum; idle = 0; continue; }
        if (++idle < 20) continue;
        fprintf(stderr, "EMU HANG: barrier sites per lane (addr2line -e %s <addr>):\n", program_invocation_name);
        for (int i = 0; i < emu_nthreads; i++) fprintf(stderr, "lane %d done=%d syncs=%llu site=%p\n", i, emu_lane_done[i], (unsigned long long)emu_sync_count[i], emu_site[i]);
        for (int l = 0; l < 2; l++) { fprintf(stderr, "ring lane %d:", l); for (int k = 0; k < 64; k++) fprintf(stderr, " %p", emu_ring[l][(emu_sync_count[l] + 1 + k) & 63]); fprintf(stderr, "\n"); }
        _exit(3);
    }
    return nullptr;
}

/* One launch: fn() on every lane of workgroup 0, then of workgroup 1, ... with threadIdx, blockIdx, gridDim and blockDim set.  A
   thread per lane for the whole launch; all lanes finish a workgroup before any starts the next.  (Workgroups never run side by
   side, so the emulator checks formats and bookkeeping, not concurrency between workgroups.) */
template <class F> struct emu_lane { unsigned lane, nblocks; const F* fn; };
template <class F> static void* emu_lane_main(void* p) {
    const emu_lane<F>* la = (const emu_lane<F>*)p;
    threadIdx.x = la->lane;
    for (unsigned b = 0; b < la->nblocks; b++) {
        blockIdx.x = b; emu_lane_done[la->lane] = 0;
        (*la->fn)();
        emu_lane_done[la->lane] = 1;
        emu_sync_count[la->lane]++; pthread_barrier_wait(&emu_barrier);
    }
    return nullptr;
}
template <class F> static void emu_launch(int nblocks, int nthreads, const F& fn) {
    static bool started = false;
    if (!started) {
        started = true;
        for (int w = 0; w < EMU_MAX_WAVES; w++) pthread_barrier_init(&emu_wbar[w], nullptr, 64);
        pthread_t wd; pthread_create(&wd, nullptr, emu_watchdog, nullptr); pthread_detach(wd);
    }
    blockDim.x = (unsigned)nthreads; gridDim.x = (unsigned)nblocks; emu_nthreads = nthreads;
    pthread_barrier_init(&emu_barrier, nullptr, (unsigned)nthreads);
    std::vector<pthread_t> th((size_t)nthreads); std::vector<emu_lane<F>> la((size_t)nthreads);
    for (int l = 0; l < nthreads; l++) { la[l].lane = (unsigned)l; la[l].nblocks = (unsigned)nblocks; la[l].fn = &fn; pthread_create(&th[l], nullptr, emu_lane_main<F>, &la[l]); }
    for (int l = 0; l < nthreads; l++) pthread_join(th[l], nullptr);
    pthread_barrier_destroy(&emu_barrier);
}

#ifdef EMU_ENCODE
#include "czstd_kernels.hip"
#include "czstd_enc.hip"

/* a compress batch as the kernels see it */
struct emu_batch {
    uint64_t n = 0; uint32_t flags = 0;
    std::vector<uint64_t> in_off, in_len, out_off, out_cap;
    uint8_t* in = nullptr; uint8_t* out = nullptr; cz_compress_result* res = nullptr;
    uint32_t* dict_index = nullptr;                                     /* (only where the file has one per buffer) */
    uint32_t counter = 0;
};
/* The buffers of batch.bin behind its header words (b->n is set): n x { u64 in_len, u64 out_cap, [u32 dict_index,] in bytes }.
   Closes f. */
static bool emu_read_batch(FILE* f, emu_batch* b, bool with_index = false) {
    const uint64_t n = b->n;
    b->in_off.resize(n); b->in_len.resize(n); b->out_off.resize(n); b->out_cap.resize(n);
    std::vector<uint32_t> idx(n ? n : 1);
    std::vector<uint8_t> in(1, 0x5A); uint64_t out_total = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t l, c; if (fread(&l, 8, 1, f) != 1 || fread(&c, 8, 1, f) != 1 || (with_index && fread(&idx[i], 4, 1, f) != 1)) return false;
        b->in_off[i] = in.size(); b->in_len[i] = l; b->out_cap[i] = c; b->out_off[i] = out_total; out_total += c;
        size_t at = in.size(); in.resize(at + l);
        if (l && fread(in.data() + at, 1, l, f) != l) return false;
    }
    fclose(f);
    b->in = (uint8_t*)malloc(in.size()); memcpy(b->in, in.data(), in.size());
    b->out = (uint8_t*)malloc(out_total ? out_total : 1); memset(b->out, 0xEE, out_total);
    b->res = (cz_compress_result*)malloc((n ? n : 1) * sizeof(cz_compress_result));
    memset(b->res, 0xA5, (n ? n : 1) * sizeof(cz_compress_result));       /* a record nobody writes shows up */
    if (with_index) { b->dict_index = (uint32_t*)malloc((n ? n : 1) * 4); memcpy(b->dict_index, idx.data(), n * 4); }
    return true;
}
/* the kernel's arguments for the batch on `scratch`, a block of `stride` bytes per workgroup */
static cz_enc_args emu_enc_args(emu_batch& b, uint8_t* scratch, size_t stride) {
    cz_enc_args a; memset(&a, 0, sizeof a);
    a.in_base = b.in; a.in_off = b.in_off.data(); a.in_len = b.in_len.data();
    a.out_base = b.out; a.out_off = b.out_off.data(); a.out_cap = b.out_cap.data(); a.results = b.res;
    a.n = (uint32_t)b.n; a.flags = b.flags; a.work_counter = &b.counter; a.scratch = scratch; a.scratch_stride = stride;
    return a;
}
/* result.bin behind the header words of the driver: n x { cz_compress_result, the whole output region }.  Closes g, frees the batch. */
static void emu_write_results(FILE* g, emu_batch* b) {
    for (uint64_t i = 0; i < b->n; i++) {
        fwrite(&b->res[i], sizeof(cz_compress_result), 1, g);
        fwrite(b->out + b->out_off[i], 1, b->out_cap[i], g);
    }
    fclose(g);
    free(b->res); free(b->out); free(b->in); free(b->dict_index);
}

/* The k dictionaries of batch.bin (k x { u64 len, dictionary bytes }), as cz_dictionary_decode and
   cz_context_set_compress_dictionaries make them: each in an exact-size block, parsed by cz_dict_setup_kernel (one workgroup of 64),
   prepared by cz_enc_dict_prep_kernel (a grid of two); the table in an exact-size block, so that a lookup out of range is an ASan
   report.  0, or the exit code of the run. */
struct emu_dicts { cze_dict_entry* table = nullptr; std::vector<void*> owned; };
static int emu_load_dicts(FILE* f, uint32_t k, emu_dicts* d) {
    d->table = (cze_dict_entry*)malloc((k ? k : 1) * sizeof(cze_dict_entry)); d->owned.push_back(d->table);
    for (uint32_t j = 0; j < k; j++) {
        uint64_t dl; if (fread(&dl, 8, 1, f) != 1) return 2;
        uint8_t* raw = (uint8_t*)malloc(dl ? dl : 1); d->owned.push_back(raw);
        if (dl && fread(raw, 1, dl, f) != dl) return 2;
        cz_device_frame_state* st = (cz_device_frame_state*)calloc(1, sizeof(cz_device_frame_state)); d->owned.push_back(st);
        uint64_t res[4] = {0, 0, 0, 0};
        emu_launch(1, 64, [&] { cz_dict_setup_kernel(raw, dl, st, res); });
        if (res[0]) { fprintf(stderr, "EMU_DICT %u: status %llu\n", j, (unsigned long long)res[0]); return 3; }
        CzeDict* img = (CzeDict*)calloc(1, sizeof(CzeDict)); d->owned.push_back(img);
        emu_launch(2, CZE_THREADS, [&] { cz_enc_dict_prep_kernel(st, raw + res[1], dl - res[1], img); });
        cze_dict_entry& e = d->table[j];
        memset(&e, 0, sizeof e);
        e.img = img; e.content = raw + res[1]; e.content_len = dl - res[1]; e.id = (uint32_t)res[2];
        for (int q = 0; q < 3; q++) e.rep[q] = st->hist[q];
    }
    return 0;
}
static void emu_free_dicts(emu_dicts* d) { for (void* p : d->owned) free(p); }
#endif
