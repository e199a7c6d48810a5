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
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

/* what the encoder needs that hip/hip_runtime.h lacks: atomicMax (32 bits for the hash table, 64 for the chain word) and the
   sleep of a poll loop */
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
#include "czstd_encrec.hip"

struct lane_arg {
    int which; unsigned lane, block;
    cz_enc_args a; cz_enc_dargs d;                                       /* which 0: the dict kernel; 3: the plain kernel */
    const uint8_t* raw; uint64_t raw_len; cz_device_frame_state* st; uint64_t* res;   /* which 1: cz_dict_setup_kernel */
    const uint8_t* content; uint64_t content_len; CzeDict* img;          /* which 2: cz_enc_dict_prep_kernel */
};
static void* lane_main(void* p) {
    lane_arg* la = (lane_arg*)p;
    threadIdx.x = la->lane; blockIdx.x = la->block;
    if (la->which == 0) cz_compress_records_dict_kernel(la->a, la->d);
    else if (la->which == 3) cz_compress_records_kernel(la->a);
    else if (la->which == 1) cz_dict_setup_kernel(la->raw, la->raw_len, la->st, la->res);
    else cz_enc_dict_prep_kernel(la->st, la->content, la->content_len, la->img);
    return nullptr;
}
static void run_lanes(const lane_arg& proto, int nthreads, int nblocks) {
    blockDim.x = (unsigned)nthreads; gridDim.x = (unsigned)nblocks;
    pthread_barrier_init(&emu_barrier, nullptr, (unsigned)nthreads);
    for (int b = 0; b < nblocks; b++) {
        std::vector<pthread_t> th((size_t)nthreads); std::vector<lane_arg> la((size_t)nthreads, proto);
        for (int l = 0; l < nthreads; l++) {
            la[l].lane = (unsigned)l; la[l].block = (unsigned)b;
            pthread_create(&th[l], nullptr, lane_main, &la[l]);
        }
        for (int l = 0; l < nthreads; l++) pthread_join(th[l], nullptr);
    }
    pthread_barrier_destroy(&emu_barrier);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    uint64_t n; uint32_t flags, k, mode;
    if (fread(&n, 8, 1, f) != 1 || fread(&flags, 4, 1, f) != 1 || fread(&k, 4, 1, f) != 1) return 2;
    { pthread_t wd; pthread_create(&wd, nullptr, emu_watchdog, nullptr); pthread_detach(wd); }
    for (int w = 0; w < EMU_MAX_WAVES; w++) pthread_barrier_init(&emu_wbar[w], nullptr, 64);
    /* the dictionaries, as cz_dictionary_decode and cz_context_set_compress_dictionaries make them */
    std::vector<cze_dict_entry> table(k);
    std::vector<void*> owned;
    for (uint32_t j = 0; j < k; j++) {
        uint64_t dl; if (fread(&dl, 8, 1, f) != 1) return 2;
        uint8_t* raw = (uint8_t*)malloc(dl ? dl : 1); owned.push_back(raw);
        if (dl && fread(raw, 1, dl, f) != dl) return 2;
        cz_device_frame_state* st = (cz_device_frame_state*)calloc(1, sizeof(cz_device_frame_state)); owned.push_back(st);
        uint64_t res[4] = {0, 0, 0, 0};
        lane_arg proto; memset(&proto, 0, sizeof proto); proto.which = 1; proto.raw = raw; proto.raw_len = dl; proto.st = st; proto.res = res;
        run_lanes(proto, 64, 1);
        if (res[0]) { fprintf(stderr, "EMU_DICT %u: status %llu\n", j, (unsigned long long)res[0]); return 3; }
        CzeDict* img = (CzeDict*)calloc(1, sizeof(CzeDict)); owned.push_back(img);
        proto.which = 2; proto.content = raw + res[1]; proto.content_len = dl - res[1]; proto.img = img;
        run_lanes(proto, CZE_THREADS, 2);
        table[j].img = img; table[j].content = raw + res[1]; table[j].content_len = dl - res[1]; table[j].id = (uint32_t)res[2];
        for (int q = 0; q < 3; q++) table[j].rep[q] = st->hist[q];
    }
    if (fread(&mode, 4, 1, f) != 1 || mode > 2 || !(flags & CZ_COMPRESS_RECORDS)) return 2;
    std::vector<uint64_t> in_off(n), in_len(n), out_off(n), out_cap(n);
    std::vector<uint32_t> idx(n ? n : 1);
    std::vector<uint8_t> in(1, 0x5A); uint64_t out_total = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t l, c; if (fread(&l, 8, 1, f) != 1 || fread(&c, 8, 1, f) != 1 || fread(&idx[i], 4, 1, f) != 1) return 2;
        in_off[i] = in.size(); in_len[i] = l; out_cap[i] = c; out_off[i] = out_total; out_total += c;
        size_t at = in.size(); in.resize(at + l);
        if (l && fread(in.data() + at, 1, l, f) != l) return 2;
    }
    fclose(f);
    uint8_t* in_exact = (uint8_t*)malloc(in.size()); memcpy(in_exact, in.data(), in.size());
    uint8_t* out = (uint8_t*)malloc(out_total ? out_total : 1); memset(out, 0xEE, out_total);
    cz_compress_result* res = (cz_compress_result*)malloc((n ? n : 1) * sizeof(cz_compress_result));
    memset(res, 0xA5, (n ? n : 1) * sizeof(cz_compress_result));          /* a record nobody writes shows up */
    cze_dict_entry* dicts = (cze_dict_entry*)malloc((k ? k : 1) * sizeof(cze_dict_entry));   /* exact size: a lookup out of range is an ASan report */
    if (k) memcpy(dicts, table.data(), k * sizeof(cze_dict_entry));
    uint32_t* dict_index = nullptr;
    if (mode == 2) { dict_index = (uint32_t*)malloc((n ? n : 1) * 4); memcpy(dict_index, idx.data(), n * 4); }
    const int grid = 2;
    uint8_t* scratch = (uint8_t*)malloc((size_t)grid * CZE_RECORDS_SCRATCH_BYTES);
    uint32_t counter = 0;
    lane_arg proto; memset(&proto, 0, sizeof proto); proto.which = mode ? 0 : 3;
    cz_enc_args& a = proto.a;
    a.in_base = in_exact; a.in_off = in_off.data(); a.in_len = in_len.data();
    a.out_base = out; a.out_off = out_off.data(); a.out_cap = out_cap.data(); a.results = res;
    a.n = (uint32_t)n; a.flags = flags; a.work_counter = &counter; a.scratch = scratch; a.scratch_stride = CZE_RECORDS_SCRATCH_BYTES;
    proto.d.dicts = dicts; proto.d.dict_index = dict_index; proto.d.ndicts = k;
    if (n) run_lanes(proto, CZE_THREADS, grid);
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    { const uint64_t mx = CZR_MAX; fwrite(&mx, 8, 1, g); }
    for (uint64_t i = 0; i < n; i++) {
        fwrite(&res[i], sizeof(cz_compress_result), 1, g);
        fwrite(out + out_off[i], 1, out_cap[i], g);
    }
    fclose(g);
    free(scratch); free(res); free(out); free(in_exact); free(dicts); free(dict_index);
    for (void* p : owned) free(p);
    return 0;
}
