/*
 * czstd_train.hip — cz_dictionary_train_*: zstd dictionaries trained on the device.
 *
 * The samples are seen as one sequence of positions 0 .. total-1 (sample after sample; cum[i] is the position of sample i's first
 * byte).  A d-mer is 8 bytes of one sample: position q has one when q + 8 does not pass the end of its sample.  Selection follows
 * fastCover with fixed parameters and integers only; every step is a launch of its own, ordered by the stream alone:
 *     cz_train_freq_kernel    freq[h(d-mer)] += 1 for every d-mer (2^20 counters, integer atomics; equal neighbours in a wave are
 *                             summed first and added once)
 *     per round r             the range r mod segments of the positions (segments equal ranges):
 *       cz_train_score_kernel   a workgroup per 256 candidate starts: hashes and counters of the positions its windows cover in LDS,
 *                               per position the nearest earlier position of the tile with the same hash, per candidate the sum of
 *                               the counters of the d-mers in its window whose nearest earlier equal lies before the window (a d-mer
 *                               counts once per window); the best (score << 32 | ~position) through LDS, then one 64-bit atomicMax per workgroup
 *       cz_train_commit_kernel  one workgroup: the winning window is put in FRONT of the content chosen so far (earlier choices end up
 *                               nearer the end: smaller offsets) and the counters of its d-mers are set to 0
 *     cz_train_concat_kernel  instead of all the above when the samples fit the content whole
 *     cz_train_image_kernel   the hash table of the content, as cz_enc_dict_prep_kernel makes it
 *     cz_train_stats_kernel   every sample parsed against the content exactly as cz_compress_frames_dict_kernel parses it (same
 *                             table, same candidates, same greedy parse, same repeat-offset rule); literals and the LL / ML / OF codes
 *                             of every parsed block go to global histograms
 *     cz_train_finish_kernel  one workgroup: every code gets its floor, Huffman code and description (cze_huf_build, cze_huf_desc),
 *                             the three FSE descriptions (czf_normalise), the header and the content behind it
 * A window is segment_len bytes, or what is left of its sample.  The dictionary depends on the samples, the capacity and the
 * parameters only: all sums are integers, all maxima have a total order.
 *
 * Needs czstd_kernels.hip, czstd_enc.hip and czstd_encfse.hip first.  Written so that the CPU SIMT emulator of tests/emu builds it
 * unchanged (tests/emu/emu_train.cpp).
 */
#define CZT_THREADS 256
#define CZT_FREQ_LOG 20
#define CZT_DMER 8u
#define CZT_TILE 256u
#define CZT_MAX_SEGMENT 4096u
#define CZT_MIN_SEGMENT 16u
#define CZT_STAGE (CZT_TILE + CZT_MAX_SEGMENT)
/* room kept for the header: magic and ID (8), the Huffman description (at most 128), the FSE descriptions (4 bits and at most
   log + 1 bits per code: 25 + 67 + 46 bytes for 21 OF, 53 ML and 36 LL codes), the repeat offsets (12) */
#define CZT_HEADER_MAX 320u
#define CZT_MAX_CONTENT (1u << 30)
#define CZT_OF_FLOOR 21u        /* offset codes 0..20: every Offset_Value of a 1 MiB window */
#define CZT_NONE 0xFFFFFFFFu

/* in HBM, zeroed before the first launch except cursor (the content capacity) */
struct cz_train_state {
    unsigned long long best;    /* of the round in hand: score << 32 | ~position; 0: nothing scored */
    uint32_t cursor;            /* the content is content[cursor, content_cap) */
    uint32_t pieces, dict_len, status;
    uint32_t lit[256];
    uint32_t seq[3][64];        /* LL, OF, ML codes (the order of czstd_encfse.hip) */
};
struct cz_train_args {
    const uint8_t* base; const uint64_t* off; const uint64_t* len;
    const uint32_t* cum;        /* n + 1 entries: cum[i] = len[0] + .. + len[i-1] */
    uint32_t n, total;
    uint32_t seg_len, segments, content_cap, dict_id;
    uint32_t* freq;             /* 2^20 */
    uint32_t* htab;             /* 2^CZE_HASH_LOG */
    uint8_t* content;           /* content_cap bytes */
    cz_train_state* st;
    uint8_t* dict;              /* the caller's buffer */
};

/* the plan both hosts (czstd_host.hip and the emulator's) launch by */
struct cz_train_plan { uint32_t content_cap, seg_len, segments, max_range, rounds; };
static inline cz_train_plan cz_train_make_plan(uint64_t dict_cap, uint32_t segment_len, uint32_t total) {
    cz_train_plan p;
    const uint64_t room = dict_cap - CZT_HEADER_MAX;
    p.content_cap = room > CZT_MAX_CONTENT ? CZT_MAX_CONTENT : (uint32_t)room;
    p.seg_len = segment_len ? segment_len : 128u;
    if (p.seg_len > p.content_cap) p.seg_len = p.content_cap;
    p.segments = p.content_cap / p.seg_len;
    p.max_range = total / p.segments + 1u;
    p.rounds = 4u * p.segments;
    return p;
}

/* the argument checks of cz_dictionary_train_* (pointers apart), shared by both hosts: the parameters ... */
static inline int cz_train_check_params(uint64_t n, uint64_t dict_cap, const cz_train_params* pr) {
    if (n == 0 || n >= 0xFFFFFFFFull || dict_cap < CZ_TRAIN_MIN_CAPACITY) return CZ_E_INVALID_ARG;
    for (int i = 0; pr && i < 6; i++) if (pr->reserved[i]) return CZ_E_INVALID_ARG;
    if (pr && pr->segment_len && (pr->segment_len < CZT_MIN_SEGMENT || pr->segment_len > CZT_MAX_SEGMENT)) return CZ_E_INVALID_ARG;
    return CZ_OK;
}
/* ... and the lengths: below 2 GiB in all, one sample with a d-mer at least.  Fills cum[0 .. n]. */
static inline int cz_train_check_lengths(const uint64_t* len, uint64_t n, uint32_t* cum) {
    uint64_t total = 0; int any = 0;
    for (uint64_t i = 0; i < n; i++) {
        cum[i] = (uint32_t)total;
        if (len[i] >= (1ull << 31)) return CZ_E_INVALID_ARG;
        total += len[i]; any |= len[i] >= CZT_DMER;
        if (total >= (1ull << 31)) return CZ_E_INVALID_ARG;
    }
    cum[n] = (uint32_t)total;
    return any ? CZ_OK : CZ_E_INVALID_ARG;
}

__device__ static inline uint32_t czt_hash(const uint8_t* p) { return (uint32_t)((cz_ld64(p) * 0xCF1BBCDCB7A56463ull) >> (64 - CZT_FREQ_LOG)); }

/* position q < total: its byte, or nullptr when it has no d-mer; *end: the position behind its sample */
__device__ static inline const uint8_t* czt_locate(const cz_train_args& a, uint32_t q, uint32_t* end) {
    uint32_t lo = 0, hi = a.n;                                          /* cum[lo] <= q < cum[hi] */
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (a.cum[mid] <= q) lo = mid; else hi = mid; }
    *end = a.cum[lo + 1];
    if (q + CZT_DMER > *end) return nullptr;
    return a.base + a.off[lo] + (q - a.cum[lo]);
}

/* ------------------------------------------------------------------ 1: frequencies */
__global__ void __launch_bounds__(CZT_THREADS) cz_train_freq_kernel(cz_train_args a) {
    const uint32_t t = threadIdx.x, lane = t & 63u;
    for (uint64_t q0 = (uint64_t)blockIdx.x * CZT_THREADS; q0 < a.total; q0 += (uint64_t)gridDim.x * CZT_THREADS) {
        const uint64_t q = q0 + t;
        uint32_t end;
        const uint8_t* p = q < a.total ? czt_locate(a, (uint32_t)q, &end) : nullptr;
        const uint32_t h = p ? czt_hash(p) : CZT_NONE;
        /* a run of equal hashes on neighbouring lanes (a run of one byte value, mostly) is added once, by its first lane */
        const uint32_t before = __shfl_up(h, 1);
        const uint64_t heads = __ballot(lane == 0 || before != h);
        if (p && ((heads >> lane) & 1u)) {
            const uint64_t later = lane == 63 ? 0ull : heads >> (lane + 1);
            atomicAdd(&a.freq[h], later ? (uint32_t)__ffsll((long long)later) : 64u - lane);
        }
    }
}

/* ------------------------------------------------------------------ 2: epochs */
struct CztShared { unsigned long long best; uint32_t hash[CZT_STAGE]; uint32_t freq[CZT_STAGE]; uint16_t prev[CZT_STAGE]; };
__shared__ CztShared czt;

__global__ void __launch_bounds__(CZT_THREADS) cz_train_score_kernel(cz_train_args a, uint32_t round) {
    const uint32_t t = threadIdx.x, L = a.seg_len;
    if (a.st->cursor < L) return;                                       /* the content is full */
    const uint32_t r = round % a.segments;
    const uint32_t lo = (uint32_t)((uint64_t)r * a.total / a.segments), hi = (uint32_t)((uint64_t)(r + 1) * a.total / a.segments);
    const uint64_t first = (uint64_t)lo + (uint64_t)blockIdx.x * CZT_TILE;
    if (first >= hi) return;
    const uint32_t s0 = (uint32_t)first;
    /* positions s0 .. s0 + R - 1: every d-mer of every window that starts in the tile */
    const uint32_t span = CZT_TILE + L - CZT_DMER, R = a.total - s0 < span ? a.total - s0 : span;
    if (t == 0) czt.best = 0;
    for (uint32_t j = t; j < R; j += CZT_THREADS) {
        uint32_t end;
        const uint8_t* p = czt_locate(a, s0 + j, &end);
        const uint32_t h = p ? czt_hash(p) : CZT_NONE;
        czt.hash[j] = h; czt.freq[j] = p ? a.freq[h] : 0u;
    }
    __syncthreads();
    /* the nearest earlier position with the same hash that a window of the tile can hold together with j */
    for (uint32_t j = t; j < R; j += CZT_THREADS) {
        const uint32_t h = czt.hash[j];
        uint32_t pv = 0xFFFFu;
        if (h != CZT_NONE && czt.freq[j]) {
            const uint32_t back = L - CZT_DMER, stop = j > back ? j - back : 0u;
            for (uint32_t i = j; i > stop; i--) if (czt.hash[i - 1] == h) { pv = i - 1; break; }
        }
        czt.prev[j] = (uint16_t)pv;
    }
    __syncthreads();
    unsigned long long mine = 0;
    if (s0 + t < hi && t < R && czt.hash[t] != CZT_NONE) {
        unsigned long long sum = 0;
        for (uint32_t k = 0; k + CZT_DMER <= L && t + k < R; k++) {
            if (czt.hash[t + k] == CZT_NONE) break;                     /* the sample ends */
            const uint32_t pv = czt.prev[t + k];
            if (pv == 0xFFFFu || pv < t) sum += czt.freq[t + k];
        }
        const uint32_t score = sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum;
        if (score) mine = ((unsigned long long)score << 32) | (uint32_t)~(s0 + t);
    }
    if (mine) atomicMax(&czt.best, mine);
    __syncthreads();
    if (t == 0 && czt.best) atomicMax(&a.st->best, czt.best);
}

__global__ void __launch_bounds__(CZT_THREADS) cz_train_commit_kernel(cz_train_args a) {
    const uint32_t t = threadIdx.x, L = a.seg_len;
    const unsigned long long best = a.st->best;
    const uint32_t cursor = a.st->cursor;
    __syncthreads();
    if (cursor < L || !(best >> 32)) { if (t == 0) a.st->best = 0; return; }
    const uint32_t s = ~(uint32_t)best;
    uint32_t end;
    const uint8_t* p = czt_locate(a, s, &end);
    const uint32_t wl = end - s < L ? end - s : L;                      /* >= 8: s has a d-mer */
    uint8_t* dst = a.content + (cursor - wl);
    for (uint32_t k = t; k < wl; k += CZT_THREADS) dst[k] = p[k];
    for (uint32_t k = t; k + CZT_DMER <= wl; k += CZT_THREADS) a.freq[czt_hash(p + k)] = 0;
    if (t == 0) { a.st->cursor = cursor - wl; a.st->best = 0; a.st->pieces++; }
}

/* the samples fit the content whole: the content is all of them, in order */
__global__ void __launch_bounds__(CZT_THREADS) cz_train_concat_kernel(cz_train_args a) {
    uint8_t* dst = a.content + (a.content_cap - a.total);
    for (uint32_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        const uint8_t* src = a.base + a.off[i];
        const uint32_t at = a.cum[i], n = a.cum[i + 1] - at;
        for (uint32_t k = threadIdx.x; k < n; k += CZT_THREADS) dst[at + k] = src[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.st->cursor = a.content_cap - a.total; a.st->pieces = a.n; }
}

/* ------------------------------------------------------------------ 3: statistics */
/* the table a frame of cz_compress_frames_dict_kernel starts from (CzeDict::htab; zeroed by the host) */
__global__ void __launch_bounds__(CZT_THREADS) cz_train_image_kernel(cz_train_args a) {
    const uint32_t cur = a.st->cursor;
    const uint8_t* content = a.content + cur;
    const uint64_t D = a.content_cap - cur, lo = D > CZE_WINDOW ? D - CZE_WINDOW : 0;
    for (uint64_t v = lo + (uint64_t)blockIdx.x * CZT_THREADS + threadIdx.x; v + 4 <= D; v += (uint64_t)gridDim.x * CZT_THREADS)
        atomicMax(&a.htab[cze_hash(cze_ld4(content + v))], (uint32_t)v + 1u);
}

struct CztHist { uint32_t lit[256]; uint32_t seq[3][64]; };
__shared__ CztHist czth;

/* Samples blockIdx.x, blockIdx.x + gridDim.x, ...: the parse of cze_frames<true> block by block (RLE blocks and blocks below 16
   bytes have none), wave 0 counting each sequence as it finds it instead of recording it. */
__global__ void __launch_bounds__(CZT_THREADS) cz_train_stats_kernel(cz_train_args a) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t cur = a.st->cursor, D = a.content_cap - cur;
    const uint8_t* dct = a.content + cur;
    for (uint32_t k = t; k < 256 + 192; k += CZT_THREADS) { if (k < 256) czth.lit[k] = 0; else czth.seq[(k - 256) >> 6][k & 63u] = 0; }
    for (uint32_t f = blockIdx.x; f < a.n; f += gridDim.x) {
        __syncthreads();
        const uint8_t* in = a.base + a.off[f];
        const uint32_t len = (uint32_t)a.len[f];
        for (uint32_t k = t; k < (1u << CZE_HASH_LOG); k += CZT_THREADS) cze.htab[k] = a.htab[k];
        uint32_t h0 = 1;                                                /* wave 0: the newest offset of the history */
        for (uint32_t b0 = 0; b0 < len;) {
            const uint32_t bsize = len - b0 < CZE_BLOCK ? len - b0 : CZE_BLOCK, b1 = b0 + bsize;
            if (t == 0) cze.rle = 1;
            __syncthreads();
            for (uint32_t k = t; k < bsize; k += CZT_THREADS) if (in[b0 + k] != in[b0]) cze.rle = 0;
            __syncthreads();
            if (!cze.rle && bsize >= 16) {
                uint32_t pp = b0, lit_start = b0;
                for (uint32_t c0 = b0; c0 < b1; c0 += CZE_CHUNK) {
                    const uint32_t p = c0 + t, valid = p + 4 <= b1;
                    const uint32_t h = valid ? cze_hash(cze_ld4(in + p)) : 0xFFFFFFFFu;
                    cze.chash[t] = h;
                    const uint32_t old = valid ? cze.htab[h] : 0;
                    __syncthreads();
                    uint32_t mlen = 0, moff = 0;
                    if (valid) {
                        const uint32_t lo = t > CZE_BACK ? t - CZE_BACK : 0;
                        for (int j = (int)t - 1; j >= (int)lo; j--) if (cze.chash[j] == h) {
                            const uint32_t m = cze_match(in, p, c0 + (uint32_t)j, b1);
                            if (m >= 4) { mlen = m; moff = t - (uint32_t)j; }
                            break;
                        }
                        if (!mlen && old && D + p - (old - 1) <= CZE_WINDOW) {
                            const uint32_t c = old - 1;
                            const uint32_t m = c < D ? cze_dmatch(dct, D, in, p, c, b1) : cze_match(in, p, c - D, b1);
                            if (m >= 4) { mlen = m; moff = D + p - c; }
                        }
                        atomicMax(&cze.htab[h], D + p + 1);
                    }
                    cze.cmlen[t] = (uint16_t)mlen; cze.cmoff[t] = moff;
                    __syncthreads();
                    if (wave == 0) {
                        const uint32_t cend = c0 + CZE_CHUNK < b1 ? c0 + CZE_CHUNK : b1;
                        while (pp < cend) {
                            const uint32_t q = pp + lane;
                            const uint64_t mask = __ballot(q < cend && cze.cmlen[q - c0] >= 4);
                            if (!mask) { pp = pp + 64 < cend ? pp + 64 : cend; continue; }
                            pp += (uint32_t)__ffsll((long long)mask) - 1;
                            uint32_t ml = cze.cmlen[pp - c0];
                            const uint32_t off = cze.cmoff[pp - c0];
                            if (ml >= CZE_CAP) {
                                for (;;) {
                                    const uint32_t rr = pp + ml + lane;
                                    const uint64_t bad = __ballot(rr >= b1 || in[rr] != cze_vb(dct, D, in, D + rr - off));
                                    if (!bad) { ml += 64; continue; }
                                    ml += (uint32_t)__ffsll((long long)bad) - 1;
                                    break;
                                }
                            }
                            const uint32_t ll = pp - lit_start;
                            for (uint32_t k = lane; k < ll; k += 64) atomicAdd(&czth.lit[in[lit_start + k]], 1u);
                            uint32_t ov;                                /* Offset_Value, as the compressor's forward pass gives it */
                            if (ll > 0 && off == h0) ov = 1; else { ov = off + 3; h0 = off; }
                            if (lane == 0) {
                                atomicAdd(&czth.seq[CZF_LL][cze_ll_code(ll)], 1u);
                                atomicAdd(&czth.seq[CZF_OF][cze_hb(ov)], 1u);
                                atomicAdd(&czth.seq[CZF_ML][cze_ml_code(ml)], 1u);
                            }
                            pp += ml; lit_start = pp;
                        }
                    }
                }
                if (wave == 0) for (uint32_t k = lit_start + lane; k < b1; k += 64) atomicAdd(&czth.lit[in[k]], 1u);
            }
            b0 = b1;
            __syncthreads();
        }
    }
    __syncthreads();
    for (uint32_t k = t; k < 256 + 192; k += CZT_THREADS) {
        const uint32_t v = k < 256 ? czth.lit[k] : czth.seq[(k - 256) >> 6][k & 63u];
        if (v) atomicAdd(k < 256 ? &a.st->lit[k] : &a.st->seq[(k - 256) >> 6][k & 63u], v);
    }
}

/* ------------------------------------------------------------------ 4: tables and header */
__global__ void __launch_bounds__(CZT_THREADS) cz_train_finish_kernel(cz_train_args a) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t cur = a.st->cursor, D = a.content_cap - cur;
    const uint8_t* content = a.content + cur;
    /* literals: every byte value counts once more than it occurred; a code for all 256, its description in the FSE-compressed form.
       While the description does not fit its 128 bytes the counts are halved (rounded up): fewer distinct weights each time.  Counts
       that are all equal would give 255 equal weights, which that form cannot write: value 0 then counts four times (a shorter code
       for certain; twice would tie with the flat code). */
    cze.hist[t] = a.st->lit[t] + 1u;
    __syncthreads();
    for (uint32_t pass = 0; pass < 80; pass++) {
        const uint32_t c = cze.hist[t];
        uint32_t flat = 1, rank = 0;
        for (uint32_t s = 0; s < 256; s++) { const uint32_t d = cze.hist[s]; flat &= d == c; rank += d < c || (d == c && s < t); }
        __syncthreads();
        if (flat) { if (t == 0) cze.hist[0] = 4u * c; __syncthreads(); continue; }
        cze.sorted[rank] = t; cze.hlen[t] = 0;
        __syncthreads();
        if (t == 0) { cze_huf_build(256); cze.huf_ok = (uint32_t)cze_huf_desc(); }
        __syncthreads();
        if (cze.huf_ok) break;
        __syncthreads();
        cze.hist[t] = (c + 1u) >> 1;
        __syncthreads();
    }
    /* sequences: floors, counts scaled below 2^22 in all (czf_normalise multiplies by up to 2^9), then the field's table */
    if (t < 192) {
        const uint32_t f = t >> 6, s = t & 63u;
        const uint32_t floors = f == CZF_LL ? 36u : (f == CZF_OF ? CZT_OF_FLOOR : 53u);
        czf.hist[f][s] = s < czf_nsym(f) ? a.st->seq[f][s] + (s < floors ? 1u : 0u) : 0u;
    }
    __syncthreads();
    if (lane == 0 && wave < 3) {
        uint32_t n;
        for (;;) {
            n = 0;
            for (uint32_t s = 0; s < 64; s++) n += czf.hist[wave][s];
            if (n < (1u << 22)) break;
            for (uint32_t s = 0; s < 64; s++) czf.hist[wave][s] = (czf.hist[wave][s] + 1u) >> 1;
        }
        czf_normalise(wave, n);
    }
    /* the ID: ZDICT's rule, from the XXH64 of the content */
    if (wave == 3) {
        const uint64_t x = cze_xxh64(content, D);
        if (lane == 0) cze.csize = a.dict_id ? a.dict_id : (uint32_t)(32768u + x % ((1ull << 31) - 32768u));
    }
    __syncthreads();
    const uint32_t hl = 8u + cze.desc_len + czf.desc_len[CZF_OF] + czf.desc_len[CZF_ML] + czf.desc_len[CZF_LL] + 12u;
    if (!cze.huf_ok || czf.desc_len[CZF_OF] > CZF_DESC_MAX || czf.desc_len[CZF_ML] > CZF_DESC_MAX || czf.desc_len[CZF_LL] > CZF_DESC_MAX ||
        hl > CZT_HEADER_MAX || D < CZT_DMER) {                          /* (never) */
        if (t == 0) { a.st->status = (uint32_t)CZ_E_UNSUPPORTED; a.st->dict_len = 0; }
        return;
    }
    if (t == 0) {
        uint8_t* o = a.dict;
        const uint32_t magic = 0xEC30A437u, id = cze.csize, rep[3] = {1u, 4u, 8u};
        uint32_t at = 0;
        for (uint32_t i = 0; i < 4; i++) o[at++] = (uint8_t)(magic >> (8 * i));
        for (uint32_t i = 0; i < 4; i++) o[at++] = (uint8_t)(id >> (8 * i));
        for (uint32_t i = 0; i < cze.desc_len; i++) o[at++] = cze.desc[i];
        const uint32_t order[3] = {CZF_OF, CZF_ML, CZF_LL};
        for (uint32_t k = 0; k < 3; k++) for (uint32_t i = 0; i < czf.desc_len[order[k]]; i++) o[at++] = czf.desc[order[k]][i];
        for (uint32_t k = 0; k < 3; k++) for (uint32_t i = 0; i < 4; i++) o[at++] = (uint8_t)(rep[k] >> (8 * i));
        a.st->dict_len = hl + D; a.st->status = 0;
    }
    for (uint32_t k = t; k < D; k += CZT_THREADS) a.dict[hl + k] = content[k];
}
