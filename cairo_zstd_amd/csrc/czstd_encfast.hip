/*
 * czstd_encfast.hip — CZ_COMPRESS_FAST: the fast compression level, one wave per block.
 *
 * cz_compress_frames_fast_kernel: a 256-thread workgroup per frame from the work counter, as cz_compress_frames_kernel, but the four
 * waves do not share a block.  The input is cut into groups of 128 KiB and each group into sub-blocks of 32 KiB; wave w of the
 * workgroup compresses sub-block w of the group in hand from start to finish, with wave-level synchronisation only, into its own
 * slot of the workgroup's scratch:
 *     RLE test; per chunk of 64 positions the hash of the 4-byte key, the nearest earlier position of the chunk with the same hash,
 *     else the wave's own table of 2^12 16-bit entries (position in the sub-block + 1), verified, measured up to CZE_CAP; the ballot
 *     parse with the extension of long matches; the literals (gather, histogram, Huffman code, description, streams with wave prefix
 *     sums); the sequences with the Predefined tables: codes and repeat offsets on a lane per sequence, the three state chains on
 *     three lanes, bit positions from a wave prefix sum, every lane OR-ing its sequence into a zeroed word buffer.
 * Every block stands alone: no match source before its sub-block, no Treeless literals, no Repeat_Mode, and Offset_Value 1 only
 * for the offset of the sequence before it in the same block (which wrote it, or repeated the one that did).  One workgroup
 * barrier per group: behind it all threads sum the four sizes, replace the group by ONE Raw block when its blocks exceed 3 + its
 * size (so a frame never exceeds cz_compress_bound), and copy it out in order.  The blocks of consecutive groups alternate between
 * two buffers of the slot, so the waves start on the next group without a second barrier.
 *
 * The frame bytes depend only on the input bytes and the flags.  Included behind czstd_encfse.hip; uses the lane-level helpers of
 * czstd_enc.hip and nothing of its shared structs, so the kernels in front of it compile as they did without it.  USER: a copy of a
 * wave-level function of its own for the kernels of czstd_encrec.hip (as for cze_sequences), so that this file's kernel compiles as it
 * did without them.
 */
#define CZQ_SUB (32u * 1024u)
#define CZQ_GROUP CZE_BLOCK
#define CZQ_HASH_LOG 12
#define CZQ_CHUNK 64u
#define CZQ_MAX_SEQ (CZQ_SUB / 4u + 64u)
#define CZQ_HUF_REGION_WORDS (((CZQ_SUB / 4u) * CZE_HUF_MAX_BITS + 31u) / 32u + 8u)   /* one stream's words */
/* a wave's slot of the workgroup's scratch in HBM: literals, sequences, the words of the Huffman streams (then of the sequence
   stream), the codes and the chain records of the sequences, two block buffers */
#define CZQ_SCR_LIT 0u
#define CZQ_SCR_SEQ (CZQ_SCR_LIT + CZQ_SUB + 256u)
#define CZQ_SCR_HUF (CZQ_SCR_SEQ + CZQ_MAX_SEQ * 8u)
#define CZQ_SCR_CODE (CZQ_SCR_HUF + 4u * CZQ_HUF_REGION_WORDS * 4u)
#define CZQ_SCR_REC (CZQ_SCR_CODE + 3u * CZQ_MAX_SEQ)
#define CZQ_SCR_BLK (CZQ_SCR_REC + 3u * CZQ_MAX_SEQ * 2u)
#define CZQ_BLK_BYTES (CZQ_SUB + 256u)
#define CZQ_SLOT_BYTES (CZQ_SCR_BLK + 2u * CZQ_BLK_BYTES)
#define CZE_FAST_SCRATCH_BYTES (CZE_WAVES * CZQ_SLOT_BYTES)
#define CZQ_NONE 0xFFFFFFFFu    /* a wave without a sub-block in the group */

/* one sequence of a sub-block: start of its match (relative to the sub-block), match length, offset, position of its first literal */
struct CzqSeq { uint16_t mstart, ml, off, lpos; };

/* A wave's LDS.  What is not live at the same time shares its bytes: the chunk arrays of the match pass with the Huffman tree, the
   literal histogram with the FSE table of the Huffman weights. */
struct CzqWave {
    union { uint16_t htab[1u << CZQ_HASH_LOG]; uint32_t htab32[1u << (CZQ_HASH_LOG - 1)]; };   /* position + 1 of the last insert; 0: empty */
    union {
        struct { uint16_t chash[CZQ_CHUNK], cmlen[CZQ_CHUNK], cmoff[CZQ_CHUNK]; } c;
        struct { uint16_t tfreq[512], tpar[512]; uint8_t tdep[512]; } t;
    } u;
    union {
        uint32_t hist[256];
        struct { uint8_t wenc[12 * 64], wsym[64], wnb[64], wbase[64]; } w;
    } v;
    uint16_t hcode[256]; uint8_t hlen[256], sorted[256];
    uint8_t desc[160];
    uint16_t cnt[34], rstart[CZE_HUF_MAX_BITS + 3];
    uint32_t desc_len, max_bits, huf_ok, bits[3], fin[3];
};
/* The workgroup's LDS: the four waves, the Predefined tables in the compact form of CzeDict (index 0 LL, 1 OF, 2 ML), the results
   of the group's blocks (type << 24 | body bytes) for two groups in flight */
struct CzqShared {
    CzqWave w[CZE_WAVES];
    uint8_t fstate[3][64], first[3][64], spread[3][64];
    int16_t dfs[3][64]; uint32_t dnb[3][64];
    uint32_t bres[2][CZE_WAVES];
    uint32_t frame, sum;
};
__shared__ CzqShared czq;

__device__ static inline uint32_t czq_log(uint32_t f) { return f == 1u ? 5u : 6u; }
__device__ static inline const int8_t* czq_norm(uint32_t f) { return f == 0u ? CZ_LL_DEFAULT : (f == 1u ? CZ_OF_DEFAULT : CZ_ML_DEFAULT); }
__device__ static inline uint32_t czq_nsym(uint32_t f) { return f == 0u ? 36u : (f == 1u ? 29u : 53u); }
__device__ static inline uint32_t czq_states(int v) { return v == -1 ? 1u : (uint32_t)v; }

/* all threads, once per kernel: the Predefined encode tables (RFC 8878 §3.1.1.3.2.2) — fstate[cumul[s] + rank] = the decoder state
   of that rank of symbol s, per symbol deltaFindState and deltaNbBits, and the lowest state, in which a stream may start */
template <int USER = 0>
__device__ static void czq_predefined() {
    const uint32_t t = threadIdx.x;
    if (t < 3) cze_fse_spread(czq_norm(t), czq_nsym(t), czq_log(t), czq.spread[t]);
    else if (t >= 64) {
        const uint32_t f = (t - 64) >> 6, s = (t - 64) & 63u;
        if (s < czq_nsym(f)) {
            const int8_t* norm = czq_norm(f);
            const uint32_t n = czq_states(norm[s]), log = czq_log(f);
            uint32_t c0 = 0;
            for (uint32_t v = 0; v < s; v++) c0 += czq_states(norm[v]);
            const uint32_t mbo = n == 1 ? log : log - cze_hb(n - 1);
            czq.dfs[f][s] = (int16_t)((int32_t)c0 - (int32_t)n);
            czq.dnb[f][s] = (mbo << 16) - (n << mbo);
        }
    }
    __syncthreads();
    if (t < 192) {
        const uint32_t f = t >> 6, u = t & 63u;
        if (u < (1u << czq_log(f))) {
            const uint32_t s = czq.spread[f][u];
            uint32_t rank = 0;
            for (uint32_t v = 0; v < u; v++) rank += czq.spread[f][v] == s;
            czq.fstate[f][(uint32_t)(czq.dfs[f][s] + (int32_t)czq_states(czq_norm(f)[s])) + rank] = (uint8_t)u;
            if (rank == 0) czq.first[f][s] = (uint8_t)u;
        }
    }
    __syncthreads();
}

/* exclusive prefix sum over the wave; the total in *total (every lane) */
__device__ static inline uint32_t czq_scan(uint32_t v, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t x = v;
    for (unsigned d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d); if (lane >= d) x += y; }
    *total = __shfl(x, 63);
    return x - v;
}
/* ORs the low n bits of v (n <= 44) into the words W at bit position o */
__device__ static inline void czq_or(uint32_t* W, uint32_t o, uint64_t v, uint32_t n) {
    if (!n) return;
    const uint32_t sh = o & 31u, i = o >> 5;
    atomicOr(&W[i], (uint32_t)(v << sh));
    if (sh + n > 32) atomicOr(&W[i + 1], (uint32_t)(v >> (32 - sh)));
    if (sh + n > 64) atomicOr(&W[i + 2], (uint32_t)(v >> (64 - sh)));
}

/* ------------------------------------------------------------------ Huffman (a wave's own) */
/* one lane: code lengths from the ranked symbols (two-queue Huffman tree), limited to 11 bits, and the canonical codes as the
   decoder assigns them (RFC 8878 §4.2.1).  S.sorted[0..n) holds the used symbols by ascending count; S.hlen is zero. */
template <int USER = 0>
__device__ static void czq_huf_build(CzqWave& S, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) S.u.t.tfreq[i] = (uint16_t)S.v.hist[S.sorted[i]];
    uint32_t li = 0, ni = n, nn = n;
    for (uint32_t k = 0; k + 1 < n; k++) {
        uint32_t a, b;
        if (li < n && (ni >= nn || S.u.t.tfreq[li] <= S.u.t.tfreq[ni])) a = li++; else a = ni++;
        if (li < n && (ni >= nn || S.u.t.tfreq[li] <= S.u.t.tfreq[ni])) b = li++; else b = ni++;
        S.u.t.tfreq[nn] = (uint16_t)(S.u.t.tfreq[a] + S.u.t.tfreq[b]); S.u.t.tpar[a] = (uint16_t)nn; S.u.t.tpar[b] = (uint16_t)nn; nn++;
    }
    S.u.t.tdep[2 * n - 2] = 0;
    for (int i = (int)(2 * n) - 3; i >= 0; i--) { const uint32_t d = S.u.t.tdep[S.u.t.tpar[i]] + 1u; S.u.t.tdep[i] = (uint8_t)(d > 32 ? 32 : d); }
    for (int i = 0; i <= 32; i++) S.cnt[i] = 0;
    for (uint32_t i = 0; i < n; i++) S.cnt[S.u.t.tdep[i]]++;
    for (int i = CZE_HUF_MAX_BITS + 1; i <= 32; i++) { S.cnt[CZE_HUF_MAX_BITS] = (uint16_t)(S.cnt[CZE_HUF_MAX_BITS] + S.cnt[i]); S.cnt[i] = 0; }
    uint32_t total = 0;
    for (uint32_t i = 1; i <= CZE_HUF_MAX_BITS; i++) total += (uint32_t)S.cnt[i] << (CZE_HUF_MAX_BITS - i);
    while (total > (1u << CZE_HUF_MAX_BITS)) {                          /* Kraft sum back to exactly 1 */
        S.cnt[CZE_HUF_MAX_BITS]--;
        for (uint32_t i = CZE_HUF_MAX_BITS - 1; i > 0; i--) if (S.cnt[i]) { S.cnt[i]--; S.cnt[i + 1] = (uint16_t)(S.cnt[i + 1] + 2); break; }
        total--;
    }
    uint32_t maxb = 0, i = n;
    for (uint32_t len = 1; len <= CZE_HUF_MAX_BITS; len++)
        for (uint32_t k = 0; k < S.cnt[len]; k++) { i--; S.hlen[S.sorted[i]] = (uint8_t)len; maxb = len; }
    S.max_bits = maxb;
    uint32_t start = 0;
    for (uint32_t w = 1; w <= maxb; w++) { S.rstart[w] = (uint16_t)start; start += (uint32_t)S.cnt[maxb + 1 - w] << (w - 1); }
    for (uint32_t s = 0; s < 256; s++) {
        const uint32_t len = S.hlen[s];
        if (!len) continue;
        const uint32_t w = maxb + 1 - len;
        S.hcode[s] = (uint16_t)(S.rstart[w] >> (w - 1)); S.rstart[w] = (uint16_t)(S.rstart[w] + (1u << (w - 1)));
    }
}
__device__ static inline uint32_t czq_hw(const CzqWave& S, uint32_t s) { const uint32_t l = S.hlen[s]; return l ? S.max_bits + 1 - l : 0u; }

/* one lane: the tree description (weights of symbols 0 .. last-1) into S.desc; direct 4-bit form up to 128 weights, FSE-compressed
   otherwise (accuracy log 6, two interleaved states).  Returns 0 when it cannot be written (the block then keeps raw literals).
   The weights' table takes the place of the histogram, which nobody reads any more. */
template <int USER = 0>
__device__ static int czq_huf_desc(CzqWave& S) {
    uint32_t last = 255;
    while (!S.hlen[last]) last--;
    const uint32_t nw = last;                                           /* weights written; the last symbol's is implied */
    if (nw <= 128) {
        S.desc[0] = (uint8_t)(127 + nw);
        for (uint32_t k = 0; k < nw; k += 2) S.desc[1 + k / 2] = (uint8_t)((czq_hw(S, k) << 4) | (k + 1 < nw ? czq_hw(S, k + 1) : 0));
        S.desc_len = 1 + (nw + 1) / 2;
        return 1;
    }
    for (int s = 0; s < 12; s++) S.cnt[s] = 0;
    for (uint32_t k = 0; k < nw; k++) S.cnt[czq_hw(S, k)]++;
    int8_t* norm = (int8_t*)&S.cnt[16];                                 /* 12 counts behind the weights' histogram */
    uint32_t distinct = 0, maxs = 0; int sum = 0;
    for (uint32_t s = 0; s < 12; s++) {
        norm[s] = 0;
        if (S.cnt[s]) { uint32_t v = (uint32_t)S.cnt[s] * 64u / nw; norm[s] = (int8_t)(v ? v : 1); distinct++; maxs = s; sum += norm[s]; }
    }
    if (distinct < 2) return 0;
    while (sum != 64) {                                                 /* the largest count absorbs the rounding */
        uint32_t big = 0;
        for (uint32_t s = 1; s < 12; s++) if (norm[s] > norm[big]) big = s;
        if (sum > 64) { if (norm[big] <= 1) return 0; norm[big]--; sum--; } else { norm[big]++; sum++; }
    }
    cze_fse_spread(norm, maxs + 1, 6, S.v.w.wsym);
    uint8_t* wfirst = (uint8_t*)&S.cnt[24];
    for (uint32_t u = 0; u < 64; u++) cze_fse_state(norm, S.v.w.wsym, 6, u, S.v.w.wnb, S.v.w.wbase, S.v.w.wenc, wfirst);
    /* table description (the decoder's read order: 4 bits of log - 5, then each probability + 1, a zero followed by 2-bit repeat
       counts of further zeros) */
    CzeBits w; w.acc = 0; w.nb = 0; w.out = S.desc + 1; w.pos = 0; w.lim = 127; w.over = 0;
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
    uint32_t st0, st1;                                                  /* the states of the even and the odd weights */
    {
        const uint32_t x = czq_hw(S, nw - 2), fl = wfirst[czq_hw(S, nw - 1)]; uint32_t u = 0;
        while (!(S.v.w.wsym[u] == x && S.v.w.wnb[u] > 0)) u++;
        if ((nw - 1) & 1) { st1 = fl; st0 = u; } else { st0 = fl; st1 = u; }
    }
    for (int k = (int)nw - 3; k >= 0; k--) {
        const uint32_t nxt = (k & 1) ? st1 : st0, u = S.v.w.wenc[czq_hw(S, (uint32_t)k) * 64 + nxt];
        cze_bits_add(b, nxt - S.v.w.wbase[u], S.v.w.wnb[u]);
        if (k & 1) st1 = u; else st0 = u;
    }
    cze_bits_add(b, st1, 6); cze_bits_add(b, st0, 6);
    const uint32_t blen = cze_bits_close(b);
    if (w.over || b.over || w.pos + blen >= 128) return 0;
    S.desc[0] = (uint8_t)(w.pos + blen);
    S.desc_len = 1 + w.pos + blen;
    return 1;
}

/* the wave: one Huffman stream of lit[s0, s1) into the words W, last literal first, four literals per lane and step; returns its
   bytes (every lane) */
template <int USER = 0>
__device__ static uint32_t czq_huf_stream(const CzqWave& S, const uint8_t* lit, uint32_t s0, uint32_t s1, uint32_t* W) {
    const uint32_t lane = threadIdx.x & 63u, n = s1 - s0;
    const uint32_t nw = (n * CZE_HUF_MAX_BITS + 32u) / 32u + 1u;
    for (uint32_t k = lane; k < nw; k += 64) W[k] = 0;
    cz_wave_sync();
    uint32_t base = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += 256) {
        const uint32_t k = t0 + 4 * lane;
        uint64_t code = 0; uint32_t len = 0;
        for (uint32_t j = 0; j < 4; j++) if (k + j < n) {
            const uint32_t sym = lit[s1 - 1 - (k + j)];
            code |= (uint64_t)S.hcode[sym] << len; len += S.hlen[sym];
        }
        uint32_t tot;
        const uint32_t o = base + czq_scan(len, &tot);
        czq_or(W, o, code, len);
        base += tot;
    }
    cz_wave_sync();
    if (lane == 0) atomicOr(&W[base >> 5], 1u << (base & 31u));         /* closing bit */
    cz_wave_sync();
    return (base >> 3) + 1;
}

/* the wave: the literals section of lit[0, nlit) at out; returns its length (every lane).  Raw, RLE or Huffman with a tree of its
   own (1 stream below 1 KiB, else 4): the rules of cze_literals without a dictionary. */
template <int USER = 0>
__device__ static uint32_t czq_literals(CzqWave& S, const uint8_t* lit, uint32_t nlit, uint8_t* out, uint32_t* hufw) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t s = lane; s < 256; s += 64) { S.v.hist[s] = 0; S.hlen[s] = 0; }
    cz_wave_sync();
    for (uint32_t k = lane; k < nlit; k += 64) atomicAdd(&S.v.hist[lit[k]], 1u);
    cz_wave_sync();
    /* rank the used symbols by (count, symbol) */
    uint32_t used = 0;
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t t = lane + 64 * j, c = S.v.hist[t];
        used += (uint32_t)__popcll(__ballot(c != 0));
        if (c) {
            uint32_t rank = 0;
            for (uint32_t s = 0; s < 256; s++) { const uint32_t d = S.v.hist[s]; rank += d && (d < c || (d == c && s < t)); }
            S.sorted[rank] = (uint8_t)t;
        }
    }
    cz_wave_sync();
    const uint32_t raw_hdr = nlit < 32 ? 1u : (nlit < 4096 ? 2u : 3u);
    if (used == 1 && nlit >= 2) {                                       /* RLE literals */
        if (lane == 0) {
            if (raw_hdr == 1) out[0] = (uint8_t)(1u | (nlit << 3));
            else if (raw_hdr == 2) { out[0] = (uint8_t)(1u | (1u << 2) | (nlit << 4)); out[1] = (uint8_t)(nlit >> 4); }
            else { out[0] = (uint8_t)(1u | (3u << 2) | (nlit << 4)); out[1] = (uint8_t)(nlit >> 4); out[2] = (uint8_t)(nlit >> 12); }
            out[raw_hdr] = lit[0];
        }
        cz_wave_sync();
        return raw_hdr + 1;
    }
    uint32_t huf_len = 0xFFFFFFFFu;
    if (used >= 2 && nlit >= 32) {
        if (lane == 0) { czq_huf_build<USER>(S, used); S.huf_ok = (uint32_t)czq_huf_desc<USER>(S); }
        cz_wave_sync();
        if (S.huf_ok) {
            const uint32_t four = nlit >= 1024, ns = four ? 4u : 1u, seg = four ? (nlit + 3) / 4 : nlit;
            uint32_t sb[4] = {0, 0, 0, 0}, sum = 0;
            for (uint32_t k = 0; k < ns; k++) {
                const uint32_t s0 = k * seg, s1 = (k + 1) * seg < nlit ? (k + 1) * seg : nlit;
                sb[k] = czq_huf_stream<USER>(S, lit, s0, s1, hufw + k * CZQ_HUF_REGION_WORDS);
                sum += sb[k];
            }
            const uint32_t dl = S.desc_len, body = dl + (four ? 6u : 0u) + sum;
            const uint32_t hdr = !four ? 3u : (nlit < 16384 && body < 16384 ? 4u : 5u);
            if (hdr + body < raw_hdr + nlit && body < (1u << 18)) {
                huf_len = hdr + body;
                if (lane == 0) {
                    const uint32_t sf = !four ? 0u : (hdr == 4 ? 2u : 3u);
                    const uint32_t bits = hdr == 3 ? 10u : (hdr == 4 ? 14u : 18u);
                    uint64_t v = 2u | (sf << 2) | ((uint64_t)nlit << 4) | ((uint64_t)body << (4 + bits));
                    for (uint32_t i = 0; i < hdr; i++) out[i] = (uint8_t)(v >> (8 * i));
                    if (four) for (uint32_t k = 0; k < 3; k++) { out[hdr + dl + 2 * k] = (uint8_t)sb[k]; out[hdr + dl + 2 * k + 1] = (uint8_t)(sb[k] >> 8); }
                }
                for (uint32_t i = lane; i < dl; i += 64) out[hdr + i] = S.desc[i];
                uint32_t at = hdr + dl + (four ? 6u : 0u);
                for (uint32_t k = 0; k < ns; k++) {
                    const uint8_t* src = (const uint8_t*)(hufw + k * CZQ_HUF_REGION_WORDS);
                    for (uint32_t i = lane; i < sb[k]; i += 64) out[at + i] = src[i];
                    at += sb[k];
                }
            }
        }
    }
    if (huf_len == 0xFFFFFFFFu) {                                       /* Raw literals */
        if (lane == 0) {
            if (raw_hdr == 1) out[0] = (uint8_t)(nlit << 3);
            else if (raw_hdr == 2) { out[0] = (uint8_t)((1u << 2) | (nlit << 4)); out[1] = (uint8_t)(nlit >> 4); }
            else { out[0] = (uint8_t)((3u << 2) | (nlit << 4)); out[1] = (uint8_t)(nlit >> 4); out[2] = (uint8_t)(nlit >> 12); }
        }
        for (uint32_t i = lane; i < nlit; i += 64) out[raw_hdr + i] = lit[i];
        huf_len = raw_hdr + nlit;
    }
    cz_wave_sync();
    return huf_len;
}

/* ------------------------------------------------------------------ sequences (a wave's own) */
/* the Offset_Value of sequence k with ll literals: 1 when it has literals and the offset of the sequence before it, which is then
   the decoder's most recent offset and was written explicitly by a sequence of this block; else offset + 3 */
__device__ static inline uint32_t czq_offset_value(const CzqSeq* sq, uint32_t k, uint32_t ll) {
    const uint32_t off = sq[k].off;
    return k > 0 && ll > 0 && sq[k - 1].off == off ? 1u : off + 3u;
}
/* the wave: the sequences section of n sequences at out[0, lim), Predefined tables; returns its length, or lim + 1 when it does not
   fit (every lane).  W: a zeroable word buffer of at least lim + 16 bytes. */
template <int USER = 0>
__device__ static uint32_t czq_sequences(CzqWave& S, const CzqSeq* sq, uint32_t n, uint32_t nlit, uint8_t* out, uint32_t lim, uint32_t* W,
                                         uint8_t* code, uint16_t* rec) {
    const uint32_t lane = threadIdx.x & 63u;
    if (n == 0) { if (lane == 0 && lim >= 1) out[0] = 0; return lim >= 1 ? 1u : lim + 1; }
    uint32_t xb = 0;
    for (uint32_t k = lane; k < n; k += 64) {
        const uint32_t ll = (k + 1 < n ? sq[k + 1].lpos : nlit) - sq[k].lpos;
        const uint32_t llc = cze_ll_code(ll), mlc = cze_ml_code(sq[k].ml), ofc = cze_hb(czq_offset_value(sq, k, ll));
        code[0 * CZQ_MAX_SEQ + k] = (uint8_t)llc; code[1 * CZQ_MAX_SEQ + k] = (uint8_t)ofc; code[2 * CZQ_MAX_SEQ + k] = (uint8_t)mlc;
        xb += CZ_LL_BITS[llc] + CZ_ML_BITS[mlc] + ofc;
    }
    uint32_t extra;
    (void)czq_scan(xb, &extra);
    cz_wave_sync();
    /* the three chains side by side: state after sequence k from the state after k + 1 and the code of k */
    if (lane < 3) {
        const uint32_t tb = lane, log = czq_log(tb), size = 1u << log;
        const uint8_t* c = code + tb * CZQ_MAX_SEQ;
        uint16_t* r = rec + tb * CZQ_MAX_SEQ;
        uint32_t s = czq.first[tb][c[n - 1]], bits = 0;
        r[n - 1] = 0;
        for (int k = (int)n - 2; k >= 0; k--) {
            const uint32_t sym = c[k], x = s + size, nb = (x + czq.dnb[tb][sym]) >> 16;
            r[k] = (uint16_t)((x & ((1u << nb) - 1u)) | (nb << 12));
            s = czq.fstate[tb][(int)(x >> nb) + czq.dfs[tb][sym]];
            bits += nb;
        }
        S.bits[tb] = bits + log; S.fin[tb] = s;
    }
    cz_wave_sync();
    const uint32_t cnt = n < 128 ? 1u : (n < 0x7F00 ? 2u : 3u), h = cnt + 1;
    const uint32_t total = extra + S.bits[0] + S.bits[1] + S.bits[2];
    if (h + (total >> 3) + 1 > lim) return lim + 1;
    if (lane == 0) {
        uint32_t p = 0;
        if (cnt == 1) out[p++] = (uint8_t)n;
        else if (cnt == 2) { out[p++] = (uint8_t)((n >> 8) + 128); out[p++] = (uint8_t)n; }
        else { out[p++] = 0xFF; out[p++] = (uint8_t)(n - 0x7F00); out[p++] = (uint8_t)((n - 0x7F00) >> 8); }
        out[p++] = 0;                                                   /* Predefined_Mode three times */
    }
    /* the bit stream, last sequence first: per sequence the OF, ML and LL state bits, then the LL, ML and OF extra bits */
    for (uint32_t k = lane; k < (total + 32u) / 32u + 2u; k += 64) W[k] = 0;
    cz_wave_sync();
    uint32_t base = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += 64) {
        const uint32_t j = t0 + lane, live = j < n, k = live ? n - 1 - j : 0;
        uint64_t a = 0, b = 0; uint32_t na = 0, nb = 0;
        if (live) {
            const uint32_t ll = (k + 1 < n ? sq[k + 1].lpos : nlit) - sq[k].lpos, ml = sq[k].ml, ov = czq_offset_value(sq, k, ll);
            const uint32_t llc = code[0 * CZQ_MAX_SEQ + k], ofc = code[1 * CZQ_MAX_SEQ + k], mlc = code[2 * CZQ_MAX_SEQ + k];
            uint32_t r = rec[1 * CZQ_MAX_SEQ + k]; a |= (uint64_t)(r & 0xFFFu) << na; na += r >> 12;
            r = rec[2 * CZQ_MAX_SEQ + k]; a |= (uint64_t)(r & 0xFFFu) << na; na += r >> 12;
            r = rec[0 * CZQ_MAX_SEQ + k]; a |= (uint64_t)(r & 0xFFFu) << na; na += r >> 12;
            a |= (uint64_t)(ll - CZ_LL_BASE[llc]) << na; na += CZ_LL_BITS[llc];
            b = ml - CZ_ML_BASE[mlc]; nb = CZ_ML_BITS[mlc];
            b |= (uint64_t)(ov - (1u << ofc)) << nb; nb += ofc;
        }
        uint32_t tot;
        const uint32_t o = base + czq_scan(na + nb, &tot);
        czq_or(W, o, a, na); czq_or(W, o + na, b, nb);
        base += tot;
    }
    cz_wave_sync();
    if (lane == 0) {                                                    /* the initial states (ML, OF, LL) and the closing bit */
        uint32_t o = base;
        czq_or(W, o, S.fin[2], 6); o += 6;
        czq_or(W, o, S.fin[1], 5); o += 5;
        czq_or(W, o, S.fin[0], 6); o += 6;
        czq_or(W, o, 1, 1);
    }
    cz_wave_sync();
    const uint32_t len = (total >> 3) + 1;
    const uint8_t* src = (const uint8_t*)W;
    for (uint32_t i = lane; i < len; i += 64) out[h + i] = src[i];
    cz_wave_sync();
    return h + len;
}

/* ------------------------------------------------------------------ one sub-block on one wave */
/* The sub-block [b0, b1) of the input, b1 > b0: RLE, Compressed (its body then in blk) or Raw, whichever is smallest.  Returns
   type << 24 | body bytes (every lane). */
template <int USER = 0>
__device__ static __forceinline__ uint32_t czq_block(CzqWave& S, const uint8_t* in, uint32_t b0, uint32_t b1, uint8_t* slot, uint8_t* blk) {
    const uint32_t lane = threadIdx.x & 63u, bsize = b1 - b0;
    uint8_t* lit = slot + CZQ_SCR_LIT;
    CzqSeq* seqs = (CzqSeq*)(slot + CZQ_SCR_SEQ);
    uint32_t* hufw = (uint32_t*)(slot + CZQ_SCR_HUF);
    /* RLE block? */
    {
        const uint32_t first = in[b0], splat = first * 0x01010101u;
        uint32_t rle = 1;
        for (uint32_t k = 0; k < bsize; k += 256) {
            const uint32_t p = k + 4 * lane;
            uint32_t bad = 0;
            if (p + 4 <= bsize) bad = cze_ld4(in + b0 + p) != splat;
            else for (uint32_t i = p; i < bsize; i++) bad |= in[b0 + i] != first;
            if (__ballot((int)bad)) { rle = 0; break; }
        }
        if (rle) return (1u << 24) | 1u;
    }
    if (bsize < 16) return bsize;
    for (uint32_t k = lane; k < (1u << (CZQ_HASH_LOG - 1)); k += 64) S.htab32[k] = 0;
    cz_wave_sync();
    /* matches, chunk by chunk, and the parse of each chunk behind them */
    uint32_t pp = b0, lit_start = b0, nseq = 0, nlit = 0;
    for (uint32_t c0 = b0; c0 < b1; c0 += CZQ_CHUNK) {
        const uint32_t p = c0 + lane, valid = p + 4 <= b1;
        const uint32_t h = valid ? cze_hash(cze_ld4(in + p)) >> (CZE_HASH_LOG - CZQ_HASH_LOG) : 0xFFFFu;
        S.u.c.chash[lane] = (uint16_t)h;
        const uint32_t old = valid ? S.htab[h] : 0;
        cz_wave_sync();
        uint32_t mlen = 0, moff = 0;
        if (valid) {
            for (int j = (int)lane - 1; j >= 0; j--) if (S.u.c.chash[j] == h) {
                const uint32_t m = cze_match<USER>(in, p, c0 + (uint32_t)j, b1);
                if (m >= 4) { mlen = m; moff = lane - (uint32_t)j; }
                break;
            }
            if (!mlen && old) {
                const uint32_t m = cze_match<USER>(in, p, b0 + old - 1, b1);
                if (m >= 4) { mlen = m; moff = p - (b0 + old - 1); }
            }
        }
        S.u.c.cmlen[lane] = (uint16_t)mlen; S.u.c.cmoff[lane] = (uint16_t)moff;
        /* the chunk into the table, highest position wins: whoever finds a lower position than its own in its entry writes again */
        const uint32_t mine = p - b0 + 1;
        for (uint32_t pending = valid;;) {
            if (pending) S.htab[h] = (uint16_t)mine;
            cz_wave_sync();
            if (pending && S.htab[h] >= mine) pending = 0;
            if (!__ballot((int)pending)) break;
        }
        const uint32_t cend = c0 + CZQ_CHUNK < b1 ? c0 + CZQ_CHUNK : b1;
        while (pp < cend) {
            const uint32_t q = pp + lane;
            const uint64_t mask = __ballot(q < cend && S.u.c.cmlen[q - c0] >= 4);
            if (!mask) { pp = pp + 64 < cend ? pp + 64 : cend; continue; }
            pp += (uint32_t)__ffsll((long long)mask) - 1;
            uint32_t ml = S.u.c.cmlen[pp - c0];
            const uint32_t off = S.u.c.cmoff[pp - c0];
            if (ml >= CZE_CAP) {
                for (;;) {
                    const uint32_t r = pp + ml + lane;
                    const uint64_t bad = __ballot(r >= b1 || in[r] != in[r - off]);
                    if (!bad) { ml += 64; continue; }
                    ml += (uint32_t)__ffsll((long long)bad) - 1;
                    break;
                }
            }
            if (lane == 0) { CzqSeq s; s.mstart = (uint16_t)(pp - b0); s.ml = (uint16_t)ml; s.off = (uint16_t)off; s.lpos = (uint16_t)nlit; seqs[nseq] = s; }
            nlit += pp - lit_start; nseq++;
            pp += ml; lit_start = pp;
        }
    }
    const uint32_t nsl = nlit;                                          /* literals of the sequences; the rest trail the last one */
    nlit += b1 - lit_start;
    cz_wave_sync();
    /* gather the literals: a lane per sequence (the last: the tail); the wave together on a run above 32 bytes */
    for (uint32_t s0 = 0; s0 <= nseq; s0 += 64) {
        const uint32_t s = s0 + lane;
        uint32_t src = 0, dst = 0, n = 0;
        if (s < nseq) { dst = seqs[s].lpos; n = (s + 1 < nseq ? seqs[s + 1].lpos : nsl) - dst; src = b0 + seqs[s].mstart - n; }
        else if (s == nseq) { dst = nsl; n = nlit - nsl; src = b1 - n; }
        if (n <= 32) for (uint32_t k = 0; k < n; k++) lit[dst + k] = in[src + k];
        for (uint64_t big = __ballot(n > 32); big; big &= big - 1) {
            const int l = __ffsll((long long)big) - 1;
            const uint32_t bn = __shfl(n, l), bsrc = __shfl(src, l), bdst = __shfl(dst, l);
            for (uint32_t k = lane; k < bn; k += 64) lit[bdst + k] = in[bsrc + k];
        }
    }
    cz_wave_sync();
    const uint32_t lsz = czq_literals<USER>(S, lit, nlit, blk, hufw);
    if (lsz < bsize) {
        const uint32_t csize = lsz + czq_sequences<USER>(S, seqs, nseq, nsl, blk + lsz, bsize - lsz, hufw, slot + CZQ_SCR_CODE, (uint16_t*)(slot + CZQ_SCR_REC));
        if (csize < bsize) return (2u << 24) | csize;
    }
    return bsize;
}

/* ------------------------------------------------------------------ the kernel */
__global__ void __launch_bounds__(CZE_THREADS, 3) cz_compress_frames_fast_kernel(cz_enc_args a) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    czq_predefined();
    uint8_t* scr = a.scratch + (uint64_t)blockIdx.x * a.scratch_stride;
    uint8_t* slot = scr + wave * CZQ_SLOT_BYTES;
    CzqWave& S = czq.w[wave];
    for (;;) {
        __syncthreads();
        if (t == 0) czq.frame = atomicAdd(a.work_counter, 1u);
        __syncthreads();
        const uint32_t f = czq.frame;
        if (f >= a.n) break;
        const uint8_t* in = a.in_base + a.in_off[f];
        const uint64_t len64 = a.in_len[f];
        uint8_t* out = a.out_base + a.out_off[f];
        const uint64_t cap = a.out_cap[f];
        cz_compress_result* res = a.results + f;
        const uint32_t cks = a.flags & CZ_COMPRESS_CHECKSUM, flags = cks | CZ_COMPRESS_FAST;
        if (len64 >= 0xFFF00000ull) {                                   /* positions are 32-bit */
            if (t == 0) { res->status = CZ_E_INVALID_ARG; res->blocks = 0; res->bytes_read = 0; res->bytes_written = 0; res->checksum = 0; res->flags = flags; }
            continue;
        }
        const uint32_t len = (uint32_t)len64;
        /* frame header */
        const uint32_t single = len <= (1u << 20);
        uint8_t hdr[14]; uint32_t hl = 0;
        hdr[hl++] = 0x28; hdr[hl++] = 0xB5; hdr[hl++] = 0x2F; hdr[hl++] = 0xFD;
        const uint32_t fcs_flag = single && len < 256 ? 0u : (len >= 256 && len < 65536 + 256 ? 1u : 2u);
        hdr[hl++] = (uint8_t)((fcs_flag << 6) | (single << 5) | (cks ? 4u : 0u));
        if (!single) hdr[hl++] = (uint8_t)((20 - 10) << 3);            /* Window_Descriptor: 1 MiB */
        if (fcs_flag == 0) hdr[hl++] = (uint8_t)len;
        else if (fcs_flag == 1) { hdr[hl++] = (uint8_t)(len - 256); hdr[hl++] = (uint8_t)((len - 256) >> 8); }
        else for (int i = 0; i < 4; i++) hdr[hl++] = (uint8_t)(len >> (8 * i));
        int status = CZ_OK; uint64_t pos = 0; uint32_t nblocks = 0, done = 0;
        if (hl <= cap) { for (uint32_t i = t; i < hl; i += CZE_THREADS) out[i] = hdr[i]; pos = hl; }
        else status = CZ_E_OUTPUT_TOO_SMALL;
        if (status == CZ_OK && len == 0) {                              /* one empty last Raw block */
            if (pos + 3 > cap) status = CZ_E_OUTPUT_TOO_SMALL;
            else { if (t < 3) out[pos + t] = t == 0 ? 1 : 0; pos += 3; nblocks = 1; }
        }
        uint32_t par = 0;
        for (uint32_t g0 = 0; status == CZ_OK && g0 < len; par ^= 1u) {
            const uint32_t g1 = len - g0 < CZQ_GROUP ? len : g0 + CZQ_GROUP, gsize = g1 - g0;
            const uint32_t s0 = g0 + wave * CZQ_SUB;
            uint32_t mine = CZQ_NONE;
            if (s0 < g1) mine = czq_block(S, in, s0, g1 - s0 < CZQ_SUB ? g1 : s0 + CZQ_SUB, slot, slot + CZQ_SCR_BLK + par * CZQ_BLK_BYTES);
            if (lane == 0) czq.bres[par][wave] = mine;
            __syncthreads();                                            /* the group's one barrier */
            uint32_t total = 0, nb = 0;
            for (uint32_t w = 0; w < CZE_WAVES; w++) { const uint32_t r = czq.bres[par][w]; if (r != CZQ_NONE) { total += 3u + (r & 0xFFFFFFu); nb++; } }
            const uint32_t raw_group = total > 3u + gsize;
            if (raw_group) { total = 3u + gsize; nb = 1; }
            if (pos + total > cap) { status = CZ_E_OUTPUT_TOO_SMALL; break; }
            const uint32_t last_group = g1 == len;
            if (raw_group) {
                const uint32_t bh = last_group | (gsize << 3);
                if (t < 3) out[pos + t] = (uint8_t)(bh >> (8 * t));
                cze_copy(out + pos + 3, in + g0, gsize);
            } else {
                uint64_t o = pos;
                for (uint32_t w = 0; w < nb; w++) {
                    const uint32_t r = czq.bres[par][w], btype = r >> 24, body = r & 0xFFFFFFu;
                    const uint32_t b0 = g0 + w * CZQ_SUB, bsize = g1 - b0 < CZQ_SUB ? g1 - b0 : CZQ_SUB;
                    const uint32_t bh = (last_group && w + 1 == nb ? 1u : 0u) | (btype << 1) | ((btype == 2 ? body : bsize) << 3);
                    if (t < 3) out[o + t] = (uint8_t)(bh >> (8 * t));
                    cze_copy(out + o + 3, btype == 2 ? scr + w * CZQ_SLOT_BYTES + CZQ_SCR_BLK + par * CZQ_BLK_BYTES : in + b0, body);
                    o += 3u + body;
                }
            }
            pos += total; nblocks += nb; done = g1;
            g0 = g1;
        }
        uint32_t sum = 0;
        if (status == CZ_OK && cks) {
            if (wave == 0) { const uint64_t x = cze_xxh64(in, len); if (t == 0) czq.sum = (uint32_t)x; }
            __syncthreads();
            sum = czq.sum;
            if (pos + 4 > cap) status = CZ_E_OUTPUT_TOO_SMALL;
            else { if (t < 4) out[pos + t] = (uint8_t)(sum >> (8 * t)); pos += 4; }
        }
        if (t == 0) {
            res->status = status; res->blocks = nblocks; res->bytes_read = done; res->bytes_written = pos;
            res->checksum = sum; res->flags = flags;
        }
    }
}
