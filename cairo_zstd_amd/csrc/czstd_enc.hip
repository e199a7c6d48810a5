/*
 * czstd_enc.hip — CDNA4 (gfx950) batched zstd compressor (cz_compress_batch_*).
 *
 * cz_compress_frames_kernel: ONE 256-thread workgroup (four waves) per frame, a persistent grid that pulls frames from an atomic
 * work counter.  The frame is cut into blocks of at most 128 KiB, processed in order; a 2^14-entry hash table of frame positions
 * (4-byte keys) stays in LDS for the whole frame, so matches reach into earlier blocks.  Per block:
 *     all threads  RLE test (every byte equal: one RLE block, nothing else)
 *     all threads  per chunk of 256 positions: hash, candidate from the table (earlier chunks) or the nearest earlier position
 *                  of the same chunk with the same hash, verified against the input in HBM, match length up to CZE_CAP; then
 *                  the chunk is inserted with atomicMax (highest position wins: the table does not depend on scheduling)
 *     wave 0       greedy parse of the chunk: ballot over 64 positions finds the next match, long matches are extended 64 bytes
 *                  per step; one record per sequence in the workgroup's scratch
 *     all waves    gather the literals; histogram (LDS atomics); lane 0 builds a length-limited (11 bits) Huffman code from the
 *                  symbols ranked in parallel; streams encoded in parallel, bit positions from a workgroup prefix sum of code
 *                  lengths, bits OR-ed into a zeroed word buffer
 *     lane 0       repeat offsets (forward), then the FSE sequence bitstream with the Predefined tables (backward)
 *     all threads  Raw, RLE or Compressed, whichever is smallest, copied to the output
 * The frame bytes depend only on the input bytes and the flags.
 *
 * cz_compress_frames_dict_kernel (cz_compress_batch_dict_*) writes the same frames against a dictionary that
 * cz_enc_dict_prep_kernel prepared once: Dictionary_ID in the header, matches into the content, the dictionary's repeat offsets,
 * Treeless literals and Repeat-mode sequence tables while the frame has not replaced them.
 *
 * CZ_COMPRESS_SPLIT (czstd_encsplit.hip, included behind this file) cuts a large input into segments that different
 * workgroups compress side by side into one frame.  Its kernel runs the same per-block pipeline from a function of its own; the two
 * kernels here keep their bodies.  cze_literals and cze_sequences carry a second template parameter only so that it gets copies of
 * its own and these kernels compile to the same code as without it.
 *
 * CZ_COMPRESS_FSE_TABLES (czstd_encfse.hip, included behind both) writes the sequences of a block with tables made
 * for that block where they make it smaller.  Its two kernels use this file's helpers up to the literals (USER = 2) and a sequence
 * writer of their own; the kernels here always use the Predefined tables (the dictionary kernel: or the dictionary's).
 *
 * Written so that the CPU SIMT emulator of tests/emu (hip/hip_runtime.h) builds it unchanged.  Needs czstd_kernels.hip first
 * (XXH64 rounds, the LL / ML code tables and the Predefined distributions).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cairo_zstd_amd.h"

#define CZE_THREADS 256
#define CZE_WAVES (CZE_THREADS / 64)
#define CZE_BLOCK (128u * 1024u)
#define CZE_HASH_LOG 14
#define CZE_CHUNK 256u
#define CZE_BACK 64            /* in-chunk look-back (positions) for a candidate with the same hash */
#define CZE_CAP 32u            /* match length the parallel pass measures; the parse extends longer ones */
#define CZE_WINDOW (1u << 20)  /* offsets never exceed 1 MiB: the window of frames that are not single-segment */
#define CZE_MAX_SEQ (CZE_BLOCK / 4u + 64u)
#define CZE_HUF_MAX_BITS 11u
#define CZE_HUF_REGION_WORDS (((CZE_BLOCK / 4u) * CZE_HUF_MAX_BITS + 31u) / 32u + 8u)   /* one stream's words */
/* per-workgroup scratch in HBM */
#define CZE_SCR_LIT 0u
#define CZE_SCR_SEQ (CZE_SCR_LIT + CZE_BLOCK + 256u)
#define CZE_SCR_HUF (CZE_SCR_SEQ + CZE_MAX_SEQ * 16u)
#define CZE_SCR_BLK (CZE_SCR_HUF + 4u * CZE_HUF_REGION_WORDS * 4u)
#define CZE_SCRATCH_BYTES (CZE_SCR_BLK + CZE_BLOCK + 4096u)

struct cz_enc_args {
    const uint8_t* in_base; const uint64_t* in_off; const uint64_t* in_len;
    uint8_t* out_base; const uint64_t* out_off; const uint64_t* out_cap;
    cz_compress_result* results;
    uint32_t n; uint32_t flags;
    uint32_t* work_counter;
    uint8_t* scratch; uint64_t scratch_stride;
};

/* one sequence of the block in hand: start of its match (block-relative), match length, offset (later: Offset_Value), position
   of its first literal in the literal buffer */
struct CzeSeq { uint32_t mstart, ml, off, lpos; };

/* The workgroup's LDS.  An FSE table for encoding is the decoder's state table (bits, baseline per state) and, per symbol, the
   state to move to for every state the decoder reaches next: enc[sym][next]. */
struct CzeShared {
    uint32_t htab[1u << CZE_HASH_LOG];                                  /* frame position + 1 of the last insert; 0: empty */
    uint32_t chash[CZE_CHUNK], cmoff[CZE_CHUNK]; uint16_t cmlen[CZE_CHUNK];
    uint32_t hist[256]; uint32_t sorted[256]; uint8_t hlen[256], hw[256]; uint16_t hcode[256];
    uint32_t tfreq[512]; uint16_t tpar[512]; uint8_t tdep[512];
    uint32_t wsum[CZE_WAVES + 1];
    uint8_t enc_ll[36 * 64], enc_ml[53 * 64], enc_of[29 * 32];
    uint8_t nb_ll[64], nb_ml[64], nb_of[32]; uint8_t base_ll[64], base_ml[64], base_of[32];
    uint8_t first_ll[36], first_ml[53], first_of[29];
    uint8_t sym_tmp[3][64];
    uint8_t wenc[12 * 64]; uint8_t wsym[64], wnb[64], wbase[64];        /* Huffman-weight FSE table */
    uint8_t desc[160];                                                 /* Huffman tree description */
    uint32_t desc_len, max_bits, huf_ok;
    uint32_t frame, rle, nseq, nseqlit, nlit, rep[3], csize;
};
__shared__ CzeShared cze;

/* A dictionary prepared for compression (cz_enc_dict_prep_kernel, once per dictionary), in HBM:
 *   htab    the frame's first hash table: entry h = 1 + the highest content position v with v + 4 <= D, D - v <= 1 MiB and
 *           hash(content[v..v+4)) = h; 0 when there is none
 *   hlen / hcode  the dictionary's Huffman code per symbol (length 0: the symbol has no code)
 *   LL / OF / ML (index 0 / 1 / 2, the decoder's order) FSE encode tables in the compact form: fstate[cumul[s] + rank] = the
 *           decoder state of that rank of symbol s; per symbol deltaFindState (cumul[s] - count), deltaNbBits and the state a
 *           stream may start in (0xFFFF: the table has no state for the symbol) */
struct CzeDict {
    uint32_t htab[1u << CZE_HASH_LOG];
    uint16_t hcode[256]; uint8_t hlen[256];
    uint16_t fstate[3][512];
    int16_t fdfs[3][64]; uint16_t ffirst[3][64]; uint32_t fdnb[3][64];
    uint32_t flog[3]; uint32_t pad;
};
/* one entry of the table a dictionary batch picks from by index (cz_context_set_compress_dictionaries) */
struct cze_dict_entry { const CzeDict* img; const uint8_t* content; uint64_t content_len; uint32_t id; uint32_t rep[3]; };
struct cz_enc_dargs { const cze_dict_entry* dicts; const uint32_t* dict_index; uint32_t ndicts; uint32_t pad; };

__device__ static inline uint32_t cze_hb(uint32_t v) { return 31u - (uint32_t)__clz((int)v); }   /* highest set bit, v > 0 */
__device__ static inline uint32_t cze_ld4(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ static inline uint32_t cze_hash(uint32_t key) { return (key * 2654435761u) >> (32 - CZE_HASH_LOG); }

/* Frames with a dictionary see one sequence of virtual positions: content byte v is v, input byte p is D + p. */
__device__ static inline uint32_t cze_vb(const uint8_t* dct, uint32_t D, const uint8_t* in, uint32_t x) { return x < D ? dct[x] : in[x - D]; }
template <int USER = 0>
__device__ static inline uint32_t cze_vld4(const uint8_t* dct, uint32_t D, const uint8_t* in, uint32_t x) {
    if (x + 4 <= D) return cze_ld4(dct + x);
    if (x >= D) return cze_ld4(in + (x - D));
    uint32_t v = 0;
    for (uint32_t i = 0; i < 4; i++) v |= cze_vb(dct, D, in, x + i) << (8 * i);
    return v;
}
/* match length at input position p against the virtual position c < D: measured against the content, across its end into the
   input; 0 when the first 4 bytes differ, at most CZE_CAP.  USER (here, for cze_vld4 and for cze_match): as for cze_sequences. */
template <int USER = 0>
__device__ static uint32_t cze_dmatch(const uint8_t* dct, uint32_t D, const uint8_t* in, uint32_t p, uint32_t c, uint32_t lim) {
    if (cze_ld4(in + p) != cze_vld4<USER>(dct, D, in, c)) return 0;
    uint32_t len = 4;
    const uint32_t cap = lim - p < CZE_CAP ? lim - p : CZE_CAP;
    while (len + 4 <= cap) {
        const uint32_t x = cze_ld4(in + p + len) ^ cze_vld4<USER>(dct, D, in, c + len);
        if (x) return len + ((uint32_t)__builtin_ctz(x) >> 3);
        len += 4;
    }
    while (len < cap && in[p + len] == cze_vb(dct, D, in, c + len)) len++;
    return len;
}

/* match length at p against c < p, both in [0, lim): 0 when the first 4 bytes differ, at most CZE_CAP */
template <int USER = 0>
__device__ static uint32_t cze_match(const uint8_t* in, uint32_t p, uint32_t c, uint32_t lim) {
    if (cze_ld4(in + p) != cze_ld4(in + c)) return 0;
    uint32_t len = 4;
    const uint32_t cap = lim - p < CZE_CAP ? lim - p : CZE_CAP;
    while (len + 4 <= cap) {
        const uint32_t x = cze_ld4(in + p + len) ^ cze_ld4(in + c + len);
        if (x) return len + ((uint32_t)__builtin_ctz(x) >> 3);
        len += 4;
    }
    while (len < cap && in[p + len] == in[c + len]) len++;
    return len;
}

/* exclusive prefix sum over the workgroup; returns the total in *total (every thread) */
__device__ static uint32_t cze_wg_scan(uint32_t v, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t x = v;
    for (unsigned d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d); if (lane >= d) x += y; }
    if (lane == 63) cze.wsum[wave] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < CZE_WAVES; w++) { const uint32_t s = cze.wsum[w]; if (w < wave) before += s; all += s; }
    __syncthreads();
    *total = all;
    return before + x - v;
}

/* ------------------------------------------------------------------ FSE tables */
/* spread symbols as the decoder does (RFC 8878 §4.1.1), then the decoder's (bits, baseline) per state and the encoder's map.
   One lane per table for the spread; the rest per state. */
__device__ static void cze_fse_spread(const int8_t* norm, uint32_t nsym, uint32_t log, uint8_t* sym) {
    const uint32_t size = 1u << log, mask = size - 1;
    uint32_t high = size - 1;
    for (uint32_t s = 0; s < nsym; s++) if (norm[s] == -1) sym[high--] = (uint8_t)s;
    const uint32_t step = (size >> 1) + (size >> 3) + 3;
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; s++)
        for (int i = 0; i < norm[s]; i++) { sym[pos] = (uint8_t)s; do pos = (pos + step) & mask; while (pos > high); }
}
/* state u (one thread each): its bits and baseline; then every next state its range covers maps back to u */
__device__ static void cze_fse_state(const int8_t* norm, const uint8_t* sym, uint32_t log, uint32_t u, uint8_t* nb, uint8_t* base,
                                     uint8_t* enc, uint8_t* first) {
    const uint32_t size = 1u << log, s = sym[u];
    uint32_t rank = 0;                                                  /* states of s before u: the decoder numbers them in order */
    for (uint32_t v = 0; v < u; v++) rank += sym[v] == s;
    const uint32_t next = (norm[s] == -1 ? 1u : (uint32_t)norm[s]) + rank;
    const uint32_t bits = log - cze_hb(next), b = (next << bits) - size;
    nb[u] = (uint8_t)bits; base[u] = (uint8_t)b;
    for (uint32_t t = b; t < b + (1u << bits); t++) enc[s * size + t] = (uint8_t)u;
    if (rank == 0) first[s] = (uint8_t)u;
}

/* ------------------------------------------------------------------ bit writer (one lane) */
struct CzeBits { uint64_t acc; uint32_t nb; uint8_t* out; uint32_t pos, lim; int over; };
__device__ static inline void cze_bits_add(CzeBits& w, uint32_t v, uint32_t n) {
    w.acc |= (uint64_t)v << w.nb; w.nb += n;
    if (w.nb >= 32) {
        if (w.pos + 4 <= w.lim) { const uint32_t lo = (uint32_t)w.acc; __builtin_memcpy(w.out + w.pos, &lo, 4); } else w.over = 1;
        w.pos += 4; w.acc >>= 32; w.nb -= 32;
    }
}
/* the closing 1 bit, then the partial bytes; returns the stream length */
__device__ static inline uint32_t cze_bits_close(CzeBits& w) {
    cze_bits_add(w, 1, 1);
    while (w.nb > 0) {
        if (w.pos < w.lim) w.out[w.pos] = (uint8_t)w.acc; else w.over = 1;
        w.pos++; w.acc >>= 8; w.nb = w.nb > 8 ? w.nb - 8 : 0;
    }
    return w.pos;
}

/* ------------------------------------------------------------------ Huffman */
/* lane 0: code lengths from the ranked symbols (two-queue Huffman tree), limited to 11 bits, weights and canonical codes as the
   decoder assigns them (RFC 8878 §4.2.1).  cze.sorted[0..n) holds the used symbols by ascending count. */
__device__ static void cze_huf_build(uint32_t n) {
    for (uint32_t i = 0; i < n; i++) cze.tfreq[i] = cze.hist[cze.sorted[i]];
    uint32_t li = 0, ni = n, nn = n;
    for (uint32_t k = 0; k + 1 < n; k++) {
        uint32_t a, b;
        if (li < n && (ni >= nn || cze.tfreq[li] <= cze.tfreq[ni])) a = li++; else a = ni++;
        if (li < n && (ni >= nn || cze.tfreq[li] <= cze.tfreq[ni])) b = li++; else b = ni++;
        cze.tfreq[nn] = cze.tfreq[a] + cze.tfreq[b]; cze.tpar[a] = (uint16_t)nn; cze.tpar[b] = (uint16_t)nn; nn++;
    }
    cze.tdep[2 * n - 2] = 0;
    for (int i = (int)(2 * n) - 3; i >= 0; i--) { const uint32_t d = cze.tdep[cze.tpar[i]] + 1u; cze.tdep[i] = (uint8_t)(d > 32 ? 32 : d); }
    uint32_t cnt[33];
    for (int i = 0; i <= 32; i++) cnt[i] = 0;
    for (uint32_t i = 0; i < n; i++) cnt[cze.tdep[i]]++;
    for (int i = CZE_HUF_MAX_BITS + 1; i <= 32; i++) { cnt[CZE_HUF_MAX_BITS] += cnt[i]; cnt[i] = 0; }
    uint32_t total = 0;
    for (uint32_t i = 1; i <= CZE_HUF_MAX_BITS; i++) total += cnt[i] << (CZE_HUF_MAX_BITS - i);
    while (total > (1u << CZE_HUF_MAX_BITS)) {                          /* Kraft sum back to exactly 1 */
        cnt[CZE_HUF_MAX_BITS]--;
        for (uint32_t i = CZE_HUF_MAX_BITS - 1; i > 0; i--) if (cnt[i]) { cnt[i]--; cnt[i + 1] += 2; break; }
        total--;
    }
    uint32_t maxb = 0, i = n;
    for (uint32_t len = 1; len <= CZE_HUF_MAX_BITS; len++)
        for (uint32_t k = 0; k < cnt[len]; k++) { i--; cze.hlen[cze.sorted[i]] = (uint8_t)len; maxb = len; }
    cze.max_bits = maxb;
    uint32_t rank_start[CZE_HUF_MAX_BITS + 2], start = 0;
    for (uint32_t w = 1; w <= maxb; w++) { rank_start[w] = start; start += cnt[maxb + 1 - w] << (w - 1); }
    for (uint32_t s = 0; s < 256; s++) {
        const uint32_t len = cze.hlen[s];
        if (!len) { cze.hw[s] = 0; continue; }
        const uint32_t w = maxb + 1 - len;
        cze.hw[s] = (uint8_t)w; cze.hcode[s] = (uint16_t)(rank_start[w] >> (w - 1)); rank_start[w] += 1u << (w - 1);
    }
}

/* lane 0: the tree description (weights of symbols 0 .. last-1) into cze.desc; direct 4-bit form up to 128 weights, FSE-compressed
   otherwise (accuracy log 6, two interleaved states).  Returns 0 when it cannot be written (the block then keeps raw literals). */
__device__ static int cze_huf_desc() {
    uint32_t last = 255;
    while (!cze.hw[last]) last--;
    const uint32_t nw = last;                                           /* weights written; the last symbol's is implied */
    if (nw <= 128) {
        cze.desc[0] = (uint8_t)(127 + nw);
        for (uint32_t k = 0; k < nw; k += 2) cze.desc[1 + k / 2] = (uint8_t)((cze.hw[k] << 4) | (k + 1 < nw ? cze.hw[k + 1] : 0));
        cze.desc_len = 1 + (nw + 1) / 2;
        return 1;
    }
    uint32_t wc[12];
    for (int s = 0; s < 12; s++) wc[s] = 0;
    for (uint32_t k = 0; k < nw; k++) wc[cze.hw[k]]++;
    int8_t norm[12]; uint32_t distinct = 0, maxs = 0; int sum = 0;
    for (uint32_t s = 0; s < 12; s++) {
        norm[s] = 0;
        if (wc[s]) { uint32_t v = wc[s] * 64u / nw; norm[s] = (int8_t)(v ? v : 1); distinct++; maxs = s; sum += norm[s]; }
    }
    if (distinct < 2) return 0;
    while (sum != 64) {                                                 /* the largest count absorbs the rounding */
        uint32_t big = 0;
        for (uint32_t s = 1; s < 12; s++) if (norm[s] > norm[big]) big = s;
        if (sum > 64) { if (norm[big] <= 1) return 0; norm[big]--; sum--; } else { norm[big]++; sum++; }
    }
    cze_fse_spread(norm, maxs + 1, 6, cze.wsym);
    uint8_t wfirst[12];
    for (uint32_t u = 0; u < 64; u++) cze_fse_state(norm, cze.wsym, 6, u, cze.wnb, cze.wbase, cze.wenc, wfirst);
    /* table description (the decoder's read order: 4 bits of log - 5, then each probability + 1, a zero followed by 2-bit repeat
       counts of further zeros) */
    CzeBits w; w.acc = 0; w.nb = 0; w.out = cze.desc + 1; w.pos = 0; w.lim = 127; w.over = 0;
    cze_bits_add(w, 6 - 5, 4);
    uint32_t counter = 0, s = 0;
    while (counter < 64) {
        const uint32_t max_rem = 64 - counter + 1, bits = cze_hb(max_rem) + 1;
        const uint32_t low = ((1u << bits) - 1u) - max_rem, mask = (1u << (bits - 1)) - 1u, value = (uint32_t)norm[s] + 1u;
        if (value < low) cze_bits_add(w, value, bits - 1);
        else cze_bits_add(w, value > mask ? value + low : value, bits);
        counter += (uint32_t)norm[s];
        if (norm[s] == 0) {
            uint32_t z = 0;
            while (s + 1 + z <= maxs && norm[s + 1 + z] == 0) z++;
            s += z;
            while (z >= 3) { cze_bits_add(w, 3, 2); z -= 3; }
            cze_bits_add(w, z, 2);
        }
        s++;
    }
    if (w.nb) { cze_bits_add(w, 0, (32 - w.nb) & 7); }                  /* to a byte boundary */
    while (w.nb) { if (w.pos < w.lim) w.out[w.pos] = (uint8_t)w.acc; else w.over = 1; w.pos++; w.acc >>= 8; w.nb -= 8; }
    /* the weights, backwards: state of the last weight any of its states, the one before it a state that reads at least one bit
       (the decoder stops when that read runs past the start of the stream) */
    CzeBits b; b.acc = 0; b.nb = 0; b.out = w.out + w.pos; b.pos = 0; b.lim = w.pos < 127 ? 127 - w.pos : 0; b.over = 0;
    uint8_t st[2];
    st[(nw - 1) & 1] = wfirst[cze.hw[nw - 1]];
    {
        const uint32_t x = cze.hw[nw - 2]; uint32_t u = 0;
        while (!(cze.wsym[u] == x && cze.wnb[u] > 0)) u++;
        st[(nw - 2) & 1] = (uint8_t)u;
    }
    for (int k = (int)nw - 3; k >= 0; k--) {
        const uint32_t nxt = st[k & 1], u = cze.wenc[cze.hw[k] * 64 + nxt];
        cze_bits_add(b, nxt - cze.wbase[u], cze.wnb[u]);
        st[k & 1] = (uint8_t)u;
    }
    cze_bits_add(b, st[1], 6); cze_bits_add(b, st[0], 6);
    const uint32_t blen = cze_bits_close(b);
    if (w.over || b.over || w.pos + blen >= 128) return 0;
    cze.desc[0] = (uint8_t)(w.pos + blen);
    cze.desc_len = 1 + w.pos + blen;
    return 1;
}

/* all threads: one Huffman stream of lit[s0, s1) into the zeroed words W, last literal first; returns its bytes (every thread) */
__device__ static uint32_t cze_huf_stream(const uint8_t* lit, uint32_t s0, uint32_t s1, uint32_t* W) {
    const uint32_t nw = ((s1 - s0) * CZE_HUF_MAX_BITS + 32u) / 32u + 1u;
    for (uint32_t k = threadIdx.x; k < nw; k += CZE_THREADS) W[k] = 0;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t t0 = 0; t0 < s1 - s0; t0 += CZE_THREADS) {
        const uint32_t k = t0 + threadIdx.x, live = k < s1 - s0;
        const uint32_t sym = live ? lit[s1 - 1 - k] : 0, len = live ? cze.hlen[sym] : 0;
        uint32_t tot;
        const uint32_t o = base + cze_wg_scan(len, &tot);
        if (live) {
            const uint32_t c = cze.hcode[sym], sh = o & 31u;
            atomicOr(&W[o >> 5], c << sh);
            if (sh + len > 32) atomicOr(&W[(o >> 5) + 1], c >> (32 - sh));
        }
        base += tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) atomicOr(&W[base >> 5], 1u << (base & 31u));  /* closing bit */
    __syncthreads();
    return (base >> 3) + 1;
}

/* ------------------------------------------------------------------ sequences (lane 0) */
__device__ static inline uint32_t cze_ll_code(uint32_t ll) {
    if (ll < 16) return ll;
    if (ll >= 64) return cze_hb(ll) + 19;
    uint32_t c = 16;
    while (c < 24 && CZ_LL_BASE[c + 1] <= ll) c++;
    return c;
}
__device__ static inline uint32_t cze_ml_code(uint32_t ml) {
    const uint32_t b = ml - 3;
    if (b < 32) return b;
    if (b >= 128) return cze_hb(b) + 36;
    uint32_t c = 32;
    while (c < 42 && CZ_ML_BASE[c + 1] <= ml) c++;
    return c;
}
/* one step of a dictionary FSE table (field f of img) for symbol `code`: from the decoder state s of the symbol after it */
__device__ static inline uint32_t cze_dfse_step(CzeBits& w, const CzeDict* img, uint32_t f, uint32_t code, uint32_t s) {
    const uint32_t x = s + (1u << img->flog[f]), nb = (x + img->fdnb[f][code]) >> 16;
    cze_bits_add(w, x & ((1u << nb) - 1u), nb);
    return img->fstate[f][(int)(x >> nb) + img->fdfs[f][code]];
}
/* the sequences section of n sequences at out[0, lim); returns its length, or lim + 1 when it does not fit.  Predefined modes;
   with a dictionary (DICT), Repeat for each field of `live` (bit 0 LL, 1 OF, 2 ML: the dictionary's table is still the decoder's)
   whose dictionary table has a state for every code of the block.  *rep_out: the fields written as Repeat.  USER: a copy of its own
   for another kernel (czstd_encsplit.hip), so that this file's kernels compile as they did without it. */
template <bool DICT, int USER = 0>
__device__ static uint32_t cze_sequences(const CzeSeq* sq, uint32_t n, uint32_t nlit, uint8_t* out, uint32_t lim, const CzeDict* img,
                                         uint32_t live, uint32_t* rep_out) {
    uint32_t h = 0, rm = 0;
    if (DICT) *rep_out = 0;
    if (n < 128) { if (lim < 1) return lim + 1; out[h++] = (uint8_t)n; }
    else if (n < 0x7F00) { if (lim < 2) return lim + 1; out[h++] = (uint8_t)((n >> 8) + 128); out[h++] = (uint8_t)n; }
    else { if (lim < 3) return lim + 1; out[h++] = 0xFF; out[h++] = (uint8_t)(n - 0x7F00); out[h++] = (uint8_t)((n - 0x7F00) >> 8); }
    if (n == 0) return h;
    if (h >= lim) return lim + 1;
    if (DICT && live) {
        rm = live;
        for (uint32_t k = 0; k < n && rm; k++) {
            const uint32_t ll = (k + 1 < n ? sq[k + 1].lpos : nlit) - sq[k].lpos;
            if (img->ffirst[0][cze_ll_code(ll)] == 0xFFFFu) rm &= ~1u;
            if (img->ffirst[1][cze_hb(sq[k].off)] == 0xFFFFu) rm &= ~2u;
            if (img->ffirst[2][cze_ml_code(sq[k].ml)] == 0xFFFFu) rm &= ~4u;
        }
        *rep_out = rm;
    }
    out[h++] = (uint8_t)((rm & 1u ? 3u << 6 : 0u) | (rm & 2u ? 3u << 4 : 0u) | (rm & 4u ? 3u << 2 : 0u));   /* Predefined or Repeat */
    CzeBits w; w.acc = 0; w.nb = 0; w.out = out + h; w.pos = 0; w.lim = lim - h; w.over = 0;
    uint32_t sLL = 0, sML = 0, sOF = 0;
    for (int k = (int)n - 1; k >= 0; k--) {
        const CzeSeq q = sq[k];
        const uint32_t ll = (k + 1 < (int)n ? sq[k + 1].lpos : nlit) - q.lpos;
        const uint32_t llc = cze_ll_code(ll), mlc = cze_ml_code(q.ml), ofc = cze_hb(q.off);
        if (k == (int)n - 1) {
            sLL = DICT && (rm & 1u) ? img->ffirst[0][llc] : cze.first_ll[llc];
            sML = DICT && (rm & 4u) ? img->ffirst[2][mlc] : cze.first_ml[mlc];
            sOF = DICT && (rm & 2u) ? img->ffirst[1][ofc] : cze.first_of[ofc];
        } else {
            uint32_t u;
            if (DICT && (rm & 2u)) sOF = cze_dfse_step(w, img, 1, ofc, sOF);
            else { u = cze.enc_of[ofc * 32 + sOF]; cze_bits_add(w, sOF - cze.base_of[u], cze.nb_of[u]); sOF = u; }
            if (DICT && (rm & 4u)) sML = cze_dfse_step(w, img, 2, mlc, sML);
            else { u = cze.enc_ml[mlc * 64 + sML]; cze_bits_add(w, sML - cze.base_ml[u], cze.nb_ml[u]); sML = u; }
            if (DICT && (rm & 1u)) sLL = cze_dfse_step(w, img, 0, llc, sLL);
            else { u = cze.enc_ll[llc * 64 + sLL]; cze_bits_add(w, sLL - cze.base_ll[u], cze.nb_ll[u]); sLL = u; }
        }
        cze_bits_add(w, ll - CZ_LL_BASE[llc], CZ_LL_BITS[llc]);
        cze_bits_add(w, q.ml - CZ_ML_BASE[mlc], CZ_ML_BITS[mlc]);
        cze_bits_add(w, q.off - (1u << ofc), ofc);
        if (w.over) return lim + 1;
    }
    cze_bits_add(w, sML, DICT && (rm & 4u) ? img->flog[2] : 6u);
    cze_bits_add(w, sOF, DICT && (rm & 2u) ? img->flog[1] : 5u);
    cze_bits_add(w, sLL, DICT && (rm & 1u) ? img->flog[0] : 6u);
    const uint32_t len = cze_bits_close(w);
    return w.over ? lim + 1 : h + len;
}

/* ------------------------------------------------------------------ XXH64 of the input (wave 0; lanes 0..3 run the accumulators) */
__device__ static uint64_t cze_xxh64(const uint8_t* p, uint64_t len) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t acc = lane == 0 ? CZ_XP1 + CZ_XP2 : (lane == 1 ? CZ_XP2 : (lane == 2 ? 0ull : 0ull - CZ_XP1));
    if (lane < 4) for (uint64_t o = 0; o + 32 <= len; o += 32) acc = cz_xxh_round(acc, cz_ld64(p + o + 8 * (uint64_t)lane));
    const uint64_t off = (len >> 5) << 5;
    uint64_t v[4];
    for (int k = 0; k < 4; k++) v[k] = (uint64_t)__shfl((uint32_t)acc, k) | ((uint64_t)__shfl((uint32_t)(acc >> 32), k) << 32);
    uint64_t h;
    if (len >= 32) {
        h = cz_rotl64(v[0], 1) + cz_rotl64(v[1], 7) + cz_rotl64(v[2], 12) + cz_rotl64(v[3], 18);
        for (int k = 0; k < 4; k++) h = cz_xxh_merge(h, v[k]);
    } else h = CZ_XP5;
    h += len;
    const uint8_t* q = p + off; const uint8_t* end = p + len;
    while (q + 8 <= end) { h ^= cz_xxh_round(0, cz_ld64(q)); h = cz_rotl64(h, 27) * CZ_XP1 + CZ_XP4; q += 8; }
    if (q + 4 <= end) { uint32_t x; __builtin_memcpy(&x, q, 4); h ^= (uint64_t)x * CZ_XP1; h = cz_rotl64(h, 23) * CZ_XP2 + CZ_XP3; q += 4; }
    while (q < end) { h ^= (uint64_t)(*q) * CZ_XP5; h = cz_rotl64(h, 11) * CZ_XP1; q++; }
    h ^= h >> 33; h *= CZ_XP2; h ^= h >> 29; h *= CZ_XP3; h ^= h >> 32;
    return h;
}

/* ------------------------------------------------------------------ one block */
/* literals section of lit[0, nlit) at out (room: lim); returns its length; Raw, RLE or Huffman (1 stream below 1 KiB, else 4).
   With a dictionary (DICT) whose Huffman code is still the decoder's table (huf_live), Treeless with that code when every symbol
   of the block has a code and the section comes out smaller.  *ltype: the Literals_Block_Type written (DICT only).  USER: as for
   cze_sequences. */
template <bool DICT, int USER = 0>
__device__ static uint32_t cze_literals(const uint8_t* lit, uint32_t nlit, uint8_t* out, uint32_t* hufw, const CzeDict* img, uint32_t huf_live,
                                        uint32_t* ltype) {
    const uint32_t t = threadIdx.x;
    for (uint32_t s = t; s < 256; s += CZE_THREADS) cze.hist[s] = 0;
    __syncthreads();
    for (uint32_t k = t; k < nlit; k += CZE_THREADS) atomicAdd(&cze.hist[lit[k]], 1u);
    __syncthreads();
    /* rank the used symbols by (count, symbol) */
    const uint32_t c = t < 256 ? cze.hist[t] : 0;
    uint32_t used, rank = 0;
    (void)cze_wg_scan(c ? 1u : 0u, &used);
    if (c) { for (uint32_t s = 0; s < 256; s++) { const uint32_t d = cze.hist[s]; rank += d && (d < c || (d == c && s < t)); } cze.sorted[rank] = t; }
    __syncthreads();
    const uint32_t raw_hdr = nlit < 32 ? 1u : (nlit < 4096 ? 2u : 3u);
    if (used == 1 && nlit >= 2) {                                       /* RLE literals */
        if (t == 0) {
            if (raw_hdr == 1) out[0] = (uint8_t)(1u | (nlit << 3));
            else if (raw_hdr == 2) { out[0] = (uint8_t)(1u | (1u << 2) | (nlit << 4)); out[1] = (uint8_t)(nlit >> 4); }
            else { out[0] = (uint8_t)(1u | (3u << 2) | (nlit << 4)); out[1] = (uint8_t)(nlit >> 4); out[2] = (uint8_t)(nlit >> 12); }
            out[raw_hdr] = lit[0];
        }
        __syncthreads();
        if (DICT) *ltype = 1;
        return raw_hdr + 1;
    }
    uint32_t huf_len = 0xFFFFFFFFu;
    if (used >= 2 && nlit >= 32) {
        if (t == 0) { for (uint32_t s = 0; s < 256; s++) cze.hlen[s] = 0; cze_huf_build(used); cze.huf_ok = (uint32_t)cze_huf_desc(); }
        __syncthreads();
        if (cze.huf_ok) {
            const uint32_t four = nlit >= 1024, ns = four ? 4u : 1u, seg = four ? (nlit + 3) / 4 : nlit;
            uint32_t sb[4] = {0, 0, 0, 0}, sum = 0;
            for (uint32_t k = 0; k < ns; k++) {
                const uint32_t s0 = k * seg, s1 = (k + 1) * seg < nlit ? (k + 1) * seg : nlit;
                sb[k] = cze_huf_stream(lit, s0, s1, hufw + k * CZE_HUF_REGION_WORDS);
                sum += sb[k];
            }
            const uint32_t body = cze.desc_len + (four ? 6u : 0u) + sum;
            const uint32_t hdr = !four ? 3u : (nlit < 16384 && body < 16384 ? 4u : 5u);
            if (hdr + body < raw_hdr + nlit && body < (1u << 18)) {
                huf_len = hdr + body;
                if (DICT) *ltype = 2;
                if (t == 0) {
                    const uint32_t sf = !four ? 0u : (hdr == 4 ? 2u : 3u);
                    const uint32_t bits = hdr == 3 ? 10u : (hdr == 4 ? 14u : 18u);
                    uint64_t v = 2u | (sf << 2) | ((uint64_t)nlit << 4) | ((uint64_t)body << (4 + bits));
                    for (uint32_t i = 0; i < hdr; i++) out[i] = (uint8_t)(v >> (8 * i));
                    for (uint32_t i = 0; i < cze.desc_len; i++) out[hdr + i] = cze.desc[i];
                    if (four) for (uint32_t k = 0; k < 3; k++) { out[hdr + cze.desc_len + 2 * k] = (uint8_t)sb[k]; out[hdr + cze.desc_len + 2 * k + 1] = (uint8_t)(sb[k] >> 8); }
                }
                uint32_t at = hdr + cze.desc_len + (four ? 6u : 0u);
                for (uint32_t k = 0; k < ns; k++) {
                    const uint8_t* src = (const uint8_t*)(hufw + k * CZE_HUF_REGION_WORDS);
                    for (uint32_t i = t; i < sb[k]; i += CZE_THREADS) out[at + i] = src[i];
                    at += sb[k];
                }
            }
        }
    }
    if (huf_len == 0xFFFFFFFFu) {                                       /* Raw literals */
        if (t == 0) {
            if (raw_hdr == 1) out[0] = (uint8_t)(nlit << 3);
            else if (raw_hdr == 2) { out[0] = (uint8_t)((1u << 2) | (nlit << 4)); out[1] = (uint8_t)(nlit >> 4); }
            else { out[0] = (uint8_t)((3u << 2) | (nlit << 4)); out[1] = (uint8_t)(nlit >> 4); out[2] = (uint8_t)(nlit >> 12); }
        }
        for (uint32_t i = t; i < nlit; i += CZE_THREADS) out[raw_hdr + i] = lit[i];
        huf_len = raw_hdr + nlit;
        if (DICT) *ltype = 0;
    }
    __syncthreads();
    if (DICT && huf_live && nlit > 0) {
        /* Treeless: the exact size from the code lengths, per stream; any symbol without a code rules it out */
        const uint32_t four = nlit >= 1024, ns = four ? 4u : 1u, seg = four ? (nlit + 3) / 4 : nlit;
        uint32_t miss = 0, acc[4] = {0, 0, 0, 0};
        if (t < 256 && cze.hist[t] && !img->hlen[t]) miss = 1;
        for (uint32_t k = t; k < nlit; k += CZE_THREADS) acc[k / seg] += img->hlen[lit[k]];
        uint32_t nmiss, bits[4] = {0, 0, 0, 0}, sum = 0;
        (void)cze_wg_scan(miss, &nmiss);
        for (uint32_t k = 0; k < ns; k++) { (void)cze_wg_scan(acc[k], &bits[k]); sum += (bits[k] >> 3) + 1; }
        const uint32_t body = (four ? 6u : 0u) + sum;
        const uint32_t hdr = !four ? 3u : (nlit < 16384 && body < 16384 ? 4u : 5u);
        if (!nmiss && hdr + body < huf_len && body < (1u << 18)) {
            for (uint32_t s = t; s < 256; s += CZE_THREADS) { cze.hlen[s] = img->hlen[s]; cze.hcode[s] = img->hcode[s]; }
            __syncthreads();
            uint32_t sb[4] = {0, 0, 0, 0};
            for (uint32_t k = 0; k < ns; k++) {
                const uint32_t s0 = k * seg, s1 = (k + 1) * seg < nlit ? (k + 1) * seg : nlit;
                sb[k] = cze_huf_stream(lit, s0, s1, hufw + k * CZE_HUF_REGION_WORDS);
            }
            if (t == 0) {
                const uint32_t sf = !four ? 0u : (hdr == 4 ? 2u : 3u);
                const uint32_t nbits = hdr == 3 ? 10u : (hdr == 4 ? 14u : 18u);
                uint64_t v = 3u | (sf << 2) | ((uint64_t)nlit << 4) | ((uint64_t)body << (4 + nbits));
                for (uint32_t i = 0; i < hdr; i++) out[i] = (uint8_t)(v >> (8 * i));
                if (four) for (uint32_t k = 0; k < 3; k++) { out[hdr + 2 * k] = (uint8_t)sb[k]; out[hdr + 2 * k + 1] = (uint8_t)(sb[k] >> 8); }
            }
            uint32_t at = hdr + (four ? 6u : 0u);
            for (uint32_t k = 0; k < ns; k++) {
                const uint8_t* src = (const uint8_t*)(hufw + k * CZE_HUF_REGION_WORDS);
                for (uint32_t i = t; i < sb[k]; i += CZE_THREADS) out[at + i] = src[i];
                at += sb[k];
            }
            huf_len = hdr + body;
            *ltype = 3;
            __syncthreads();
        }
    }
    return huf_len;
}

/* ------------------------------------------------------------------ the kernel */
__global__ void __launch_bounds__(CZE_THREADS) cz_compress_frames_kernel(cz_enc_args a) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    /* Predefined tables (RFC 8878 §3.1.1.3.2.2): spread by lanes 0..2, then one thread per state */
    if (t < 3) {
        if (t == 0) cze_fse_spread(CZ_LL_DEFAULT, 36, 6, cze.sym_tmp[0]);
        else if (t == 1) cze_fse_spread(CZ_ML_DEFAULT, 53, 6, cze.sym_tmp[1]);
        else cze_fse_spread(CZ_OF_DEFAULT, 29, 5, cze.sym_tmp[2]);
    }
    __syncthreads();
    if (t < 64) cze_fse_state(CZ_LL_DEFAULT, cze.sym_tmp[0], 6, t, cze.nb_ll, cze.base_ll, cze.enc_ll, cze.first_ll);
    else if (t < 128) cze_fse_state(CZ_ML_DEFAULT, cze.sym_tmp[1], 6, t - 64, cze.nb_ml, cze.base_ml, cze.enc_ml, cze.first_ml);
    else if (t < 160) cze_fse_state(CZ_OF_DEFAULT, cze.sym_tmp[2], 5, t - 128, cze.nb_of, cze.base_of, cze.enc_of, cze.first_of);
    uint8_t* scr = a.scratch + (uint64_t)blockIdx.x * a.scratch_stride;
    uint8_t* lit = scr + CZE_SCR_LIT;
    CzeSeq* seqs = (CzeSeq*)(scr + CZE_SCR_SEQ);
    uint32_t* hufw = (uint32_t*)(scr + CZE_SCR_HUF);
    uint8_t* blk = scr + CZE_SCR_BLK;
    for (;;) {
        __syncthreads();
        if (t == 0) cze.frame = atomicAdd(a.work_counter, 1u);
        __syncthreads();
        const uint32_t f = cze.frame;
        if (f >= a.n) break;
        const uint8_t* in = a.in_base + a.in_off[f];
        const uint64_t len64 = a.in_len[f];
        uint8_t* out = a.out_base + a.out_off[f];
        const uint64_t cap = a.out_cap[f];
        cz_compress_result* res = a.results + f;
        const uint32_t flags = a.flags & CZ_COMPRESS_CHECKSUM;
        if (len64 >= 0xFFF00000ull) {                                   /* positions are 32-bit */
            if (t == 0) { res->status = CZ_E_INVALID_ARG; res->blocks = 0; res->bytes_read = 0; res->bytes_written = 0; res->checksum = 0; res->flags = flags; }
            continue;
        }
        const uint32_t len = (uint32_t)len64;
        for (uint32_t k = t; k < (1u << CZE_HASH_LOG); k += CZE_THREADS) cze.htab[k] = 0;
        if (t == 0) { cze.rep[0] = 1; cze.rep[1] = 4; cze.rep[2] = 8; }
        /* frame header */
        const uint32_t single = len <= (1u << 20);
        uint8_t hdr[14]; uint32_t hl = 0;
        hdr[hl++] = 0x28; hdr[hl++] = 0xB5; hdr[hl++] = 0x2F; hdr[hl++] = 0xFD;
        const uint32_t fcs_flag = single && len < 256 ? 0u : (len >= 256 && len < 65536 + 256 ? 1u : 2u);
        hdr[hl++] = (uint8_t)((fcs_flag << 6) | (single << 5) | (flags ? 4u : 0u));
        if (!single) hdr[hl++] = (uint8_t)((20 - 10) << 3);            /* Window_Descriptor: 1 MiB */
        if (fcs_flag == 0) hdr[hl++] = (uint8_t)len;
        else if (fcs_flag == 1) { hdr[hl++] = (uint8_t)(len - 256); hdr[hl++] = (uint8_t)((len - 256) >> 8); }
        else for (int i = 0; i < 4; i++) hdr[hl++] = (uint8_t)(len >> (8 * i));
        int status = CZ_OK; uint64_t pos = 0; uint32_t nblocks = 0, done = 0;
        if (hl <= cap) { for (uint32_t i = t; i < hl; i += CZE_THREADS) out[i] = hdr[i]; pos = hl; }
        else status = CZ_E_OUTPUT_TOO_SMALL;
        for (uint32_t b0 = 0; status == CZ_OK && (b0 < len || (len == 0 && nblocks == 0));) {
            const uint32_t bsize = len - b0 < CZE_BLOCK ? len - b0 : CZE_BLOCK, b1 = b0 + bsize, last = b1 == len;
            /* RLE block? */
            if (t == 0) cze.rle = bsize > 0;
            __syncthreads();
            for (uint32_t k = t; k < bsize; k += CZE_THREADS) if (in[b0 + k] != in[b0]) cze.rle = 0;
            __syncthreads();
            const uint32_t rle = cze.rle;
            uint32_t btype = 0, csize = 0;                              /* 0 Raw, 1 RLE, 2 Compressed */
            if (rle) btype = 1;
            else if (bsize >= 16) {
                /* matches, chunk by chunk; wave 0 parses each chunk behind the parallel pass */
                uint32_t pp = b0, lit_start = b0, nseq = 0, nlit = 0;
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
                        if (!mlen && old && p - (old - 1) <= CZE_WINDOW) {
                            const uint32_t m = cze_match(in, p, old - 1, b1);
                            if (m >= 4) { mlen = m; moff = p - (old - 1); }
                        }
                        atomicMax(&cze.htab[h], p + 1);
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
                                    const uint32_t r = pp + ml + lane;
                                    const uint64_t bad = __ballot(r >= b1 || in[r] != in[r - off]);
                                    if (!bad) { ml += 64; continue; }
                                    ml += (uint32_t)__ffsll((long long)bad) - 1;
                                    break;
                                }
                            }
                            if (lane == 0) { CzeSeq s; s.mstart = pp - b0; s.ml = ml; s.off = off; s.lpos = nlit; seqs[nseq] = s; }
                            nlit += pp - lit_start; nseq++;
                            pp += ml; lit_start = pp;
                        }
                    }
                }
                if (t == 0) { cze.nseq = nseq; cze.nseqlit = nlit; cze.nlit = nlit + (b1 - lit_start); }
                __syncthreads();
                nseq = cze.nseq; nlit = cze.nlit;
                const uint32_t nsl = cze.nseqlit;                       /* literals of the sequences; the rest trail the last one */
                /* gather the literals: a wave per sequence, then the tail */
                for (uint32_t s = wave; s <= nseq; s += CZE_WAVES) {
                    uint32_t src, dst, n;
                    if (s < nseq) { const CzeSeq q = seqs[s]; dst = q.lpos; n = (s + 1 < nseq ? seqs[s + 1].lpos : nsl) - dst; src = b0 + q.mstart - n; }
                    else { dst = nsl; n = nlit - nsl; src = b1 - n; }
                    for (uint32_t k = lane; k < n; k += 64) lit[dst + k] = in[src + k];
                }
                __syncthreads();
                /* repeat offsets, forward (only the case Offset_Value 1 with literals: the history then stays) */
                const uint32_t r0 = cze.rep[0], r1 = cze.rep[1], r2 = cze.rep[2];
                if (t == 0) {
                    uint32_t h0 = r0, h1 = r1, h2 = r2;
                    for (uint32_t s = 0; s < nseq; s++) {
                        const uint32_t ll = (s + 1 < nseq ? seqs[s + 1].lpos : nsl) - seqs[s].lpos, off = seqs[s].off;
                        if (ll > 0 && off == h0) seqs[s].off = 1;
                        else { seqs[s].off = off + 3; h2 = h1; h1 = h0; h0 = off; }
                    }
                    cze.rep[0] = h0; cze.rep[1] = h1; cze.rep[2] = h2;
                }
                __syncthreads();
                const uint32_t lsz = cze_literals<false>(lit, nlit, blk, hufw, nullptr, 0u, nullptr);
                if (lsz < bsize) {
                    if (t == 0) cze.csize = lsz + cze_sequences<false>(seqs, nseq, nsl, blk + lsz, bsize - lsz, nullptr, 0u, nullptr);
                    __syncthreads();
                    csize = cze.csize;
                    if (csize < bsize) btype = 2;
                }
                if (btype != 2) {                                       /* the decoder will not see these sequences */
                    __syncthreads();
                    if (t == 0) { cze.rep[0] = r0; cze.rep[1] = r1; cze.rep[2] = r2; }
                }
            }
            const uint32_t body = btype == 0 ? bsize : (btype == 1 ? 1u : csize);
            if (pos + 3 + body > cap) { status = CZ_E_OUTPUT_TOO_SMALL; break; }
            const uint32_t bh = last | (btype << 1) | ((btype == 2 ? csize : bsize) << 3);
            if (t == 0) { out[pos] = (uint8_t)bh; out[pos + 1] = (uint8_t)(bh >> 8); out[pos + 2] = (uint8_t)(bh >> 16); }
            const uint8_t* src = btype == 0 ? in + b0 : (btype == 1 ? in + b0 : blk);
            for (uint32_t i = t; i < body; i += CZE_THREADS) out[pos + 3 + i] = src[i];
            pos += 3 + body; nblocks++; done = b1;
            b0 = b1;
            __syncthreads();
        }
        uint32_t sum = 0;
        if (status == CZ_OK && flags) {
            if (wave == 0) { const uint64_t x = cze_xxh64(in, len); if (t == 0) cze.csize = (uint32_t)x; }
            __syncthreads();
            sum = cze.csize;
            if (pos + 4 > cap) status = CZ_E_OUTPUT_TOO_SMALL;
            else { if (t < 4) out[pos + t] = (uint8_t)(sum >> (8 * t)); pos += 4; }
        }
        if (t == 0) {
            res->status = status; res->blocks = nblocks; res->bytes_read = done; res->bytes_written = pos;
            res->checksum = sum; res->flags = flags;
        }
    }
}

/* ------------------------------------------------------------------ the kernels */
/* The body of cz_compress_frames_dict_kernel: frame i starts from dictionary d.dicts[d.dict_index[i]] or, for
   CZ_COMPRESS_NO_DICT, from nothing, and then comes out exactly as cz_compress_frames_kernel writes it.  With DICT = false it is
   that kernel's code; the plain kernel keeps its own copy above all the same, because inlining this body into it changed its
   resources (the compiler promoted the header array to LDS: 3.5 KB more, 9 more SGPR spills). */
template <bool DICT>
__device__ static __forceinline__ void cze_frames(cz_enc_args a, cz_enc_dargs d) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    /* Predefined tables (RFC 8878 §3.1.1.3.2.2): spread by lanes 0..2, then one thread per state */
    if (t < 3) {
        if (t == 0) cze_fse_spread(CZ_LL_DEFAULT, 36, 6, cze.sym_tmp[0]);
        else if (t == 1) cze_fse_spread(CZ_ML_DEFAULT, 53, 6, cze.sym_tmp[1]);
        else cze_fse_spread(CZ_OF_DEFAULT, 29, 5, cze.sym_tmp[2]);
    }
    __syncthreads();
    if (t < 64) cze_fse_state(CZ_LL_DEFAULT, cze.sym_tmp[0], 6, t, cze.nb_ll, cze.base_ll, cze.enc_ll, cze.first_ll);
    else if (t < 128) cze_fse_state(CZ_ML_DEFAULT, cze.sym_tmp[1], 6, t - 64, cze.nb_ml, cze.base_ml, cze.enc_ml, cze.first_ml);
    else if (t < 160) cze_fse_state(CZ_OF_DEFAULT, cze.sym_tmp[2], 5, t - 128, cze.nb_of, cze.base_of, cze.enc_of, cze.first_of);
    uint8_t* scr = a.scratch + (uint64_t)blockIdx.x * a.scratch_stride;
    uint8_t* lit = scr + CZE_SCR_LIT;
    CzeSeq* seqs = (CzeSeq*)(scr + CZE_SCR_SEQ);
    uint32_t* hufw = (uint32_t*)(scr + CZE_SCR_HUF);
    uint8_t* blk = scr + CZE_SCR_BLK;
    for (;;) {
        __syncthreads();
        if (t == 0) cze.frame = atomicAdd(a.work_counter, 1u);
        __syncthreads();
        const uint32_t f = cze.frame;
        if (f >= a.n) break;
        const uint8_t* in = a.in_base + a.in_off[f];
        const uint64_t len64 = a.in_len[f];
        uint8_t* out = a.out_base + a.out_off[f];
        const uint64_t cap = a.out_cap[f];
        cz_compress_result* res = a.results + f;
        const uint32_t flags = a.flags & CZ_COMPRESS_CHECKSUM;
        const CzeDict* img = nullptr; const uint8_t* dct = nullptr; uint64_t dlen = 0; uint32_t did = 0, bad_index = 0;
        if (DICT) {
            const uint32_t di = d.dict_index ? d.dict_index[f] : 0u;
            if (di != CZ_COMPRESS_NO_DICT) {
                if (di >= d.ndicts) bad_index = 1;
                else { const cze_dict_entry& e = d.dicts[di]; img = e.img; dct = e.content; dlen = e.content_len; did = e.id; }
            }
        }
        if (len64 + dlen >= 0xFFF00000ull || bad_index) {               /* (virtual) positions are 32-bit */
            if (t == 0) { res->status = CZ_E_INVALID_ARG; res->blocks = 0; res->bytes_read = 0; res->bytes_written = 0; res->checksum = 0; res->flags = flags; }
            continue;
        }
        const uint32_t len = (uint32_t)len64, D = DICT ? (uint32_t)dlen : 0u;
        if (DICT && img) {                                              /* the table starts as the dictionary's */
            for (uint32_t k = t; k < (1u << CZE_HASH_LOG) / 4u; k += CZE_THREADS) {
                const uint4 v = ((const uint4*)img->htab)[k];
                cze.htab[4 * k] = v.x; cze.htab[4 * k + 1] = v.y; cze.htab[4 * k + 2] = v.z; cze.htab[4 * k + 3] = v.w;
            }
            if (t == 0) { const cze_dict_entry& e = d.dicts[d.dict_index ? d.dict_index[f] : 0u]; cze.rep[0] = e.rep[0]; cze.rep[1] = e.rep[1]; cze.rep[2] = e.rep[2]; }
        } else {
            for (uint32_t k = t; k < (1u << CZE_HASH_LOG); k += CZE_THREADS) cze.htab[k] = 0;
            if (t == 0) { cze.rep[0] = 1; cze.rep[1] = 4; cze.rep[2] = 8; }
        }
        /* which of the dictionary's tables are still the decoder's: its Huffman table (every thread), its LL / OF / ML tables
           (bits 0..2; lane 0 writes the sequences) */
        uint32_t huf_live = DICT && img, fse_live = DICT && img ? 7u : 0u;
        /* frame header */
        const uint32_t single = len <= (1u << 20);
        uint8_t hdr[14]; uint32_t hl = 0;
        hdr[hl++] = 0x28; hdr[hl++] = 0xB5; hdr[hl++] = 0x2F; hdr[hl++] = 0xFD;
        const uint32_t fcs_flag = single && len < 256 ? 0u : (len >= 256 && len < 65536 + 256 ? 1u : 2u);
        const uint32_t idb = !DICT || !img || did == 0 || (a.flags & CZ_COMPRESS_NO_DICT_ID) ? 0u : (did < 256 ? 1u : (did < 65536 ? 2u : 4u));
        hdr[hl++] = (uint8_t)((fcs_flag << 6) | (single << 5) | (flags ? 4u : 0u) | (idb == 4 ? 3u : idb));
        if (!single) hdr[hl++] = (uint8_t)((20 - 10) << 3);            /* Window_Descriptor: 1 MiB */
        for (uint32_t i = 0; i < idb; i++) hdr[hl++] = (uint8_t)(did >> (8 * i));   /* Dictionary_ID: the smallest field that holds it */
        if (fcs_flag == 0) hdr[hl++] = (uint8_t)len;
        else if (fcs_flag == 1) { hdr[hl++] = (uint8_t)(len - 256); hdr[hl++] = (uint8_t)((len - 256) >> 8); }
        else for (int i = 0; i < 4; i++) hdr[hl++] = (uint8_t)(len >> (8 * i));
        int status = CZ_OK; uint64_t pos = 0; uint32_t nblocks = 0, done = 0;
        if (hl <= cap) { for (uint32_t i = t; i < hl; i += CZE_THREADS) out[i] = hdr[i]; pos = hl; }
        else status = CZ_E_OUTPUT_TOO_SMALL;
        for (uint32_t b0 = 0; status == CZ_OK && (b0 < len || (len == 0 && nblocks == 0));) {
            const uint32_t bsize = len - b0 < CZE_BLOCK ? len - b0 : CZE_BLOCK, b1 = b0 + bsize, last = b1 == len;
            /* RLE block? */
            if (t == 0) cze.rle = bsize > 0;
            __syncthreads();
            for (uint32_t k = t; k < bsize; k += CZE_THREADS) if (in[b0 + k] != in[b0]) cze.rle = 0;
            __syncthreads();
            const uint32_t rle = cze.rle;
            uint32_t btype = 0, csize = 0;                              /* 0 Raw, 1 RLE, 2 Compressed */
            if (rle) btype = 1;
            else if (bsize >= 16) {
                /* matches, chunk by chunk; wave 0 parses each chunk behind the parallel pass */
                uint32_t pp = b0, lit_start = b0, nseq = 0, nlit = 0;
                for (uint32_t c0 = b0; c0 < b1; c0 += CZE_CHUNK) {
                    const uint32_t p = c0 + t, valid = p + 4 <= b1;
                    const uint32_t h = valid ? cze_hash(cze_ld4(in + p)) : 0xFFFFFFFFu;
                    cze.chash[t] = h;
                    const uint32_t old = valid ? cze.htab[h] : 0;     /* (virtual) position + 1 */
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
                            const uint32_t m = DICT && c < D ? cze_dmatch(dct, D, in, p, c, b1) : cze_match(in, p, c - D, b1);
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
                                    const uint32_t r = pp + ml + lane;
                                    const uint64_t bad = __ballot(r >= b1 || in[r] != (DICT ? cze_vb(dct, D, in, D + r - off) : in[r - off]));
                                    if (!bad) { ml += 64; continue; }
                                    ml += (uint32_t)__ffsll((long long)bad) - 1;
                                    break;
                                }
                            }
                            if (lane == 0) { CzeSeq s; s.mstart = pp - b0; s.ml = ml; s.off = off; s.lpos = nlit; seqs[nseq] = s; }
                            nlit += pp - lit_start; nseq++;
                            pp += ml; lit_start = pp;
                        }
                    }
                }
                if (t == 0) { cze.nseq = nseq; cze.nseqlit = nlit; cze.nlit = nlit + (b1 - lit_start); }
                __syncthreads();
                nseq = cze.nseq; nlit = cze.nlit;
                const uint32_t nsl = cze.nseqlit;                       /* literals of the sequences; the rest trail the last one */
                /* gather the literals: a wave per sequence, then the tail */
                for (uint32_t s = wave; s <= nseq; s += CZE_WAVES) {
                    uint32_t src, dst, n;
                    if (s < nseq) { const CzeSeq q = seqs[s]; dst = q.lpos; n = (s + 1 < nseq ? seqs[s + 1].lpos : nsl) - dst; src = b0 + q.mstart - n; }
                    else { dst = nsl; n = nlit - nsl; src = b1 - n; }
                    for (uint32_t k = lane; k < n; k += 64) lit[dst + k] = in[src + k];
                }
                __syncthreads();
                /* repeat offsets, forward (only the case Offset_Value 1 with literals: the history then stays) */
                const uint32_t r0 = cze.rep[0], r1 = cze.rep[1], r2 = cze.rep[2];
                if (t == 0) {
                    uint32_t h0 = r0, h1 = r1, h2 = r2;
                    for (uint32_t s = 0; s < nseq; s++) {
                        const uint32_t ll = (s + 1 < nseq ? seqs[s + 1].lpos : nsl) - seqs[s].lpos, off = seqs[s].off;
                        if (ll > 0 && off == h0) seqs[s].off = 1;
                        else { seqs[s].off = off + 3; h2 = h1; h1 = h0; h0 = off; }
                    }
                    cze.rep[0] = h0; cze.rep[1] = h1; cze.rep[2] = h2;
                }
                __syncthreads();
                uint32_t ltype = 0, srep = 0;
                const uint32_t lsz = cze_literals<DICT>(lit, nlit, blk, hufw, img, huf_live, &ltype);
                if (lsz < bsize) {
                    if (t == 0) cze.csize = lsz + cze_sequences<DICT>(seqs, nseq, nsl, blk + lsz, bsize - lsz, img, fse_live, &srep);
                    __syncthreads();
                    csize = cze.csize;
                    if (csize < bsize) btype = 2;
                }
                if (btype != 2) {                                       /* the decoder will not see these sequences */
                    __syncthreads();
                    if (t == 0) { cze.rep[0] = r0; cze.rep[1] = r1; cze.rep[2] = r2; }
                } else if (DICT) {                                      /* ... and only a Compressed block changes its tables */
                    if (ltype == 2) huf_live = 0;
                    if (nseq) fse_live &= srep;
                }
            }
            const uint32_t body = btype == 0 ? bsize : (btype == 1 ? 1u : csize);
            if (pos + 3 + body > cap) { status = CZ_E_OUTPUT_TOO_SMALL; break; }
            const uint32_t bh = last | (btype << 1) | ((btype == 2 ? csize : bsize) << 3);
            if (t == 0) { out[pos] = (uint8_t)bh; out[pos + 1] = (uint8_t)(bh >> 8); out[pos + 2] = (uint8_t)(bh >> 16); }
            const uint8_t* src = btype == 0 ? in + b0 : (btype == 1 ? in + b0 : blk);
            for (uint32_t i = t; i < body; i += CZE_THREADS) out[pos + 3 + i] = src[i];
            pos += 3 + body; nblocks++; done = b1;
            b0 = b1;
            __syncthreads();
        }
        uint32_t sum = 0;
        if (status == CZ_OK && flags) {
            if (wave == 0) { const uint64_t x = cze_xxh64(in, len); if (t == 0) cze.csize = (uint32_t)x; }
            __syncthreads();
            sum = cze.csize;
            if (pos + 4 > cap) status = CZ_E_OUTPUT_TOO_SMALL;
            else { if (t < 4) out[pos + t] = (uint8_t)(sum >> (8 * t)); pos += 4; }
        }
        if (t == 0) {
            res->status = status; res->blocks = nblocks; res->bytes_read = done; res->bytes_written = pos;
            res->checksum = sum; res->flags = flags;
        }
    }
}

/* cz_compress_batch_dict_*: the same frames, each from its dictionary (or none) */
__global__ void __launch_bounds__(CZE_THREADS) cz_compress_frames_dict_kernel(cz_enc_args a, cz_enc_dargs d) {
    cze_frames<true>(a, d);
}

/* Prepares a dictionary for compression (CzeDict, zeroed by the host): every workgroup inserts its share of the content positions
   into the hash table (atomicMax: the highest position wins whatever the schedule); workgroup 0 also derives the Huffman code
   from the decoder's table and the compact FSE encode tables from the decoder's LL / OF / ML tables (cz_dict_setup_kernel). */
__global__ void __launch_bounds__(CZE_THREADS) cz_enc_dict_prep_kernel(const cz_device_frame_state* st, const uint8_t* content, uint64_t D,
                                                                        CzeDict* img) {
    const uint32_t t = threadIdx.x;
    const uint64_t lo = D > CZE_WINDOW ? D - CZE_WINDOW : 0;
    for (uint64_t v = lo + (uint64_t)blockIdx.x * CZE_THREADS + t; v + 4 <= D; v += (uint64_t)gridDim.x * CZE_THREADS)
        atomicMax(&img->htab[cze_hash(cze_ld4(content + v))], (uint32_t)v + 1u);
    if (blockIdx.x != 0) return;
    /* huf[] holds symbol | length << 8 per cell of 2^max_bits; a symbol's code is the index of its first cell >> (max_bits - length) */
    const uint32_t mb = st->huf_max_bits;
    for (uint32_t i = t; mb && i < (1u << mb); i += CZE_THREADS) {
        const uint32_t e = st->huf[i], s = e & 0xFFu, l = (e >> 8) & 15u;
        if (l && l <= mb && !(i & ((1u << (mb - l)) - 1u))) { img->hlen[s] = (uint8_t)l; img->hcode[s] = (uint16_t)(i >> (mb - l)); }
    }
    if (t < 3) {                                                        /* one lane per table: count, cumulate, rank in state order */
        const uint32_t log = st->fse_log[t], size = 1u << log;
        uint32_t cnt[64], cum[64];
        for (uint32_t s = 0; s < 64; s++) cnt[s] = 0;
        for (uint32_t u = 0; u < size; u++) cnt[(st->fse[t][u] >> 24) & 63u]++;
        uint32_t c = 0;
        for (uint32_t s = 0; s < 64; s++) { cum[s] = c; c += cnt[s]; }
        for (uint32_t u = 0; u < size; u++) { const uint32_t s = (st->fse[t][u] >> 24) & 63u; img->fstate[t][cum[s]++] = (uint16_t)u; }
        for (uint32_t s = 0; s < 64; s++) {
            const uint32_t n = cnt[s], c0 = cum[s] - n;
            if (!n) { img->ffirst[t][s] = 0xFFFFu; img->fdfs[t][s] = 0; img->fdnb[t][s] = 0; continue; }
            const uint32_t mbo = n == 1 ? log : log - cze_hb(n - 1);
            img->fdfs[t][s] = (int16_t)((int32_t)c0 - (int32_t)n);
            img->fdnb[t][s] = (mbo << 16) - (n << mbo);
            img->ffirst[t][s] = img->fstate[t][c0];
        }
        img->flog[t] = log;
    }
}
