/*
 * czstd_encfse.hip — CZ_COMPRESS_FSE_TABLES: sequences sections with per-block FSE tables.
 *
 * The frames are those of czstd_enc.hip (and, with CZ_COMPRESS_SPLIT, of czstd_encsplit.hip) except for the sequences section of
 * a Compressed block: each of LL, OF and ML independently takes Predefined_Mode, RLE_Mode (every sequence of the block has the same
 * code for the field) or FSE_Compressed_Mode with a table made from the block's own histogram, whichever makes the section
 * smallest.  The comparison is exact: description bytes plus the field's state bits, initial state included; ties go to Predefined,
 * then to RLE.  Repeat_Mode is never written, so no table state crosses a block and a segment cut needs no rule of its own.
 *
 * Per block, behind the parse and the repeat-offset pass (czf_sequences, all 256 threads):
 *     all threads   one thread per sequence: the LL / ML / OF codes (bytes in the workgroup's scratch), their histograms (LDS atomics),
 *                   the sum of the extra bits
 *     3 lanes       first lane of waves 0..2, one field each: accuracy log, normalised counts, table description (czf_normalise)
 *     all threads   the block's encode tables in the compact form of CzeDict (fstate[cumul[s] + rank], deltaFindState, deltaNbBits):
 *                   the spread on one lane per table, the per-symbol values on a thread per symbol, the ranks on a thread per state.
 *                   The Predefined tables are built the same way once per kernel.
 *     6 lanes       wave 0: the state chains of (Predefined, own) x (LL, OF, ML) side by side; each stores (value, nbits) per
 *                   sequence in scratch and sums its bits: the exact sizes
 *     lane 0        the modes, the section header and the descriptions
 *     all threads   bit position of every sequence from a workgroup prefix sum (last sequence first); each thread ORs its sequence's
 *                   state bits and extra bits into a zeroed word buffer; lane 0 adds the initial states and the closing bit
 *
 * Accuracy log of a field with U >= 2 used codes in a block of n sequences: max(5, floor(log2 n) - 2), raised until 2^log >= U,
 * at most 9 (LL, ML) or 8 (OF).  Normalisation to T = 2^log: a code with count c gets round(c T / n) states, or the "less than 1"
 * probability (-1, one state) when c T < n; the most frequent code (the lowest on a tie) takes what is missing from T; while the
 * sum exceeds T the code with the most states (the lowest on a tie) gives one up.  Both are functions of the histogram alone.
 *
 * cz_compress_frames_fse_kernel is cz_compress_frames_kernel, cz_compress_segments_fse_kernel is cz_compress_segments_kernel (same
 * plan kernel, same chain word, same progress argument), each around czf_block.  They have copies of their own of everything:
 * the kernels of czstd_enc.hip and czstd_encsplit.hip compile as they did without this file.  Included behind czstd_encsplit.hip.
 * USER (czf_sequences, czf_predefined and what they call): as for cze_sequences, a copy of its own for a kernel of a later file
 * (czstd_enchigh.hip: 1), so that a second caller changes no inlining decision in the two kernels here.
 */
#define CZF_LL 0u
#define CZF_OF 1u
#define CZF_ML 2u
#define CZF_DESC_MAX 96u        /* a description: 4 bits, then at most 10 bits per code and 2 per run of three unused ones */
/* extra scratch per workgroup, behind the scratch of the kernel it extends: the codes of the block's sequences, one byte array per
   field, and the (value | nbits << 12) records of the six chains */
#define CZF_SCR_CODE 0u
#define CZF_SCR_REC (CZF_SCR_CODE + 3u * CZE_MAX_SEQ)
#define CZF_SCR_BYTES (CZF_SCR_REC + 6u * CZE_MAX_SEQ * 2u + 256u)
#define CZE_FSE_SCRATCH_BYTES (CZE_SCRATCH_BYTES + CZF_SCR_BYTES)
#define CZE_FSE_SPLIT_SCRATCH_BYTES (CZE_SPLIT_SCRATCH_BYTES + CZF_SCR_BYTES)

/* table 2 f + own: field f (the decoder's order: LL, OF, ML), own = 0 Predefined, 1 made from the block in hand */
struct CzfShared {
    uint32_t hist[3][64];
    int16_t norm[3][64];
    uint16_t fstate[6][512];
    int16_t dfs[6][64]; uint16_t first[6][64]; uint32_t dnb[6][64];
    uint8_t spread[3][512];
    uint8_t desc[3][CZF_DESC_MAX];
    uint32_t log[6], bits[6], fin[6];                                   /* per chain: its bits (initial state included), its last state */
    uint32_t desc_len[3], used[3], only[3], mode[3];
    uint32_t hdr, total, fail;
};
__shared__ CzfShared czf;

__device__ static inline uint32_t czf_nsym(uint32_t f) { return f == CZF_LL ? 36u : (f == CZF_OF ? 32u : 53u); }
__device__ static inline uint32_t czf_maxlog(uint32_t f) { return f == CZF_OF ? 8u : 9u; }
__device__ static inline uint32_t czf_states(int v) { return v == -1 ? 1u : (uint32_t)v; }

/* one lane: spreads the symbols as the decoder does (RFC 8878 §4.1.1) */
template <int USER = 0> __device__ static void czf_spread(const int16_t* norm, uint32_t nsym, uint32_t log, uint8_t* sym) {
    const uint32_t size = 1u << log, mask = size - 1;
    uint32_t high = size - 1;
    for (uint32_t s = 0; s < nsym; s++) if (norm[s] == -1) sym[high--] = (uint8_t)s;
    const uint32_t step = (size >> 1) + (size >> 3) + 3;
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; s++)
        for (int i = 0; i < norm[s]; i++) { sym[pos] = (uint8_t)s; do pos = (pos + step) & mask; while (pos > high); }
}
/* one thread per symbol: deltaFindState and deltaNbBits */
template <int USER = 0> __device__ static void czf_symbol(uint32_t tb, const int16_t* norm, uint32_t s, uint32_t log) {
    const uint32_t n = czf_states(norm[s]);
    uint32_t c0 = 0;
    for (uint32_t v = 0; v < s; v++) c0 += czf_states(norm[v]);
    if (!n) { czf.dfs[tb][s] = 0; czf.dnb[tb][s] = 0; czf.first[tb][s] = 0xFFFFu; return; }
    const uint32_t mbo = n == 1 ? log : log - cze_hb(n - 1);
    czf.dfs[tb][s] = (int16_t)((int32_t)c0 - (int32_t)n);
    czf.dnb[tb][s] = (mbo << 16) - (n << mbo);
}
/* one thread per state u: the states of a symbol in increasing order; a stream may start in the lowest */
template <int USER = 0> __device__ static void czf_state(uint32_t tb, const int16_t* norm, const uint8_t* sym, uint32_t u) {
    const uint32_t s = sym[u];
    uint32_t rank = 0;
    for (uint32_t v = 0; v < u; v++) rank += sym[v] == s;
    czf.fstate[tb][(uint32_t)(czf.dfs[tb][s] + (int32_t)czf_states(norm[s])) + rank] = (uint16_t)u;
    if (rank == 0) czf.first[tb][s] = (uint16_t)u;
}
/* all threads: tables 2 f + own of the fields in `active` from czf.norm[f] and czf.log[2 f + own] */
template <int USER = 0> __device__ static void czf_build(uint32_t own, uint32_t active) {
    const uint32_t t = threadIdx.x;
    if (t < 3) { if ((active >> t) & 1u) czf_spread<USER>(czf.norm[t], czf_nsym(t), czf.log[2 * t + own], czf.spread[t]); }
    else if (t >= 64) {
        const uint32_t f = (t - 64) >> 6, s = (t - 64) & 63u;
        if (((active >> f) & 1u) && s < czf_nsym(f)) czf_symbol<USER>(2 * f + own, czf.norm[f], s, czf.log[2 * f + own]);
    }
    __syncthreads();
    for (uint32_t f = 0; f < 3; f++) if ((active >> f) & 1u)
        for (uint32_t u = t; u < (1u << czf.log[2 * f + own]); u += CZE_THREADS) czf_state<USER>(2 * f + own, czf.norm[f], czf.spread[f], u);
    __syncthreads();
}
/* all threads, once per kernel: the Predefined tables (RFC 8878 §3.1.1.3.2.2) */
template <int USER = 0> __device__ static void czf_predefined() {
    const uint32_t t = threadIdx.x;
    if (t < 64) {
        czf.norm[CZF_LL][t] = t < 36 ? CZ_LL_DEFAULT[t] : 0;
        czf.norm[CZF_OF][t] = t < 29 ? CZ_OF_DEFAULT[t] : 0;
        czf.norm[CZF_ML][t] = t < 53 ? CZ_ML_DEFAULT[t] : 0;
    }
    if (t == 0) { czf.log[2 * CZF_LL] = 6; czf.log[2 * CZF_OF] = 5; czf.log[2 * CZF_ML] = 6; }
    __syncthreads();
    czf_build<USER>(0u, 7u);
}

/* one lane: field f of a block of n sequences from czf.hist[f] — the used codes, and for two or more the accuracy log, the
   normalised counts and the table description (the forward bit stream of RFC 8878 §4.1.1) */
template <int USER = 0> __device__ static void czf_normalise(uint32_t f, uint32_t n) {
    const uint32_t nsym = czf_nsym(f);
    uint32_t used = 0, maxs = 0, big = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        const uint32_t c = czf.hist[f][s];
        if (c) { used++; maxs = s; if (c > czf.hist[f][big]) big = s; }
    }
    czf.used[f] = used; czf.only[f] = maxs; czf.desc_len[f] = 0;
    if (used < 2) return;
    uint32_t log = cze_hb(n) >= 7 ? cze_hb(n) - 2 : 5;
    while ((1u << log) < used) log++;
    if (log > czf_maxlog(f)) log = czf_maxlog(f);
    czf.log[2 * f + 1] = log;
    const uint32_t T = 1u << log;
    int16_t* norm = czf.norm[f];
    uint32_t sum = 0;
    for (uint32_t s = 0; s < 64; s++) {
        const uint32_t c = s < nsym ? czf.hist[f][s] : 0;               /* c T < 2^25 */
        const int v = !c ? 0 : (c * T < n ? -1 : (int)((c * T + n / 2) / n));
        norm[s] = (int16_t)v; sum += czf_states(v);
    }
    if (sum < T) { norm[big] = (int16_t)(norm[big] + (int)(T - sum)); sum = T; }
    while (sum > T) {                                                   /* T >= used: some code holds two states or more */
        uint32_t m = 0;
        for (uint32_t s = 1; s <= maxs; s++) if (norm[s] > norm[m]) m = s;
        norm[m]--; sum--;
    }
    CzeBits w; w.acc = 0; w.nb = 0; w.out = czf.desc[f]; w.pos = 0; w.lim = CZF_DESC_MAX; w.over = 0;
    cze_bits_add(w, log - 5, 4);
    uint32_t rem = T, s = 0;
    while (rem > 0) {
        const uint32_t max_rem = rem + 1, bits = cze_hb(max_rem) + 1;
        const uint32_t low = ((1u << bits) - 1u) - max_rem, mask = (1u << (bits - 1)) - 1u, value = (uint32_t)(norm[s] + 1);
        if (value < low) cze_bits_add(w, value, bits - 1);
        else cze_bits_add(w, value > mask ? value + low : value, bits);
        rem -= czf_states(norm[s]);
        if (norm[s] == 0) {
            uint32_t z = 0;
            while (s + 1 + z <= maxs && norm[s + 1 + z] == 0) z++;
            s += z;
            while (z >= 3) { cze_bits_add(w, 3, 2); z -= 3; }
            cze_bits_add(w, z, 2);
        }
        s++;
    }
    if (w.nb) cze_bits_add(w, 0, (32 - w.nb) & 7);                      /* the last byte is padded */
    while (w.nb) { if (w.pos < w.lim) w.out[w.pos] = (uint8_t)w.acc; else w.over = 1; w.pos++; w.acc >>= 8; w.nb -= 8; }
    czf.desc_len[f] = w.over ? 0xFFFFu : w.pos;                         /* (never: CZF_DESC_MAX holds the longest) */
}

/* ORs the low n bits of v (n <= 42) into the words W at bit position o */
__device__ static inline void czf_or(uint32_t* W, uint32_t o, uint64_t v, uint32_t n) {
    if (!n) return;
    const uint32_t sh = o & 31u, i = o >> 5;
    atomicOr(&W[i], (uint32_t)(v << sh));
    if (sh + n > 32) atomicOr(&W[i + 1], (uint32_t)(v >> (32 - sh)));
    if (sh + n > 64) atomicOr(&W[i + 2], (uint32_t)(v >> (64 - sh)));
}

/* all threads: the sequences section of n sequences at out[0, lim); returns its length, or lim + 1 when it does not fit (every
   thread).  W: a zeroable word buffer of at least lim + 16 bytes; fscr: the CZF_SCR_* scratch. */
template <int USER = 0> __device__ static uint32_t czf_sequences(const CzeSeq* sq, uint32_t n, uint32_t nlit, uint8_t* out, uint32_t lim, uint32_t* W, uint8_t* fscr) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    if (n == 0) { if (t == 0 && lim >= 1) out[0] = 0; return lim >= 1 ? 1u : lim + 1; }
    uint8_t* code = fscr + CZF_SCR_CODE;
    uint16_t* rec = (uint16_t*)(fscr + CZF_SCR_REC);
    /* codes, histograms, extra bits */
    if (t < 192) czf.hist[t >> 6][t & 63u] = 0;
    __syncthreads();
    uint32_t xb = 0;
    for (uint32_t k = t; k < n; k += CZE_THREADS) {
        const CzeSeq q = sq[k];
        const uint32_t ll = (k + 1 < n ? sq[k + 1].lpos : nlit) - q.lpos;
        const uint32_t llc = cze_ll_code(ll), mlc = cze_ml_code(q.ml), ofc = cze_hb(q.off);
        code[CZF_LL * CZE_MAX_SEQ + k] = (uint8_t)llc; code[CZF_OF * CZE_MAX_SEQ + k] = (uint8_t)ofc; code[CZF_ML * CZE_MAX_SEQ + k] = (uint8_t)mlc;
        atomicAdd(&czf.hist[CZF_LL][llc], 1u); atomicAdd(&czf.hist[CZF_OF][ofc], 1u); atomicAdd(&czf.hist[CZF_ML][mlc], 1u);
        xb += CZ_LL_BITS[llc] + CZ_ML_BITS[mlc] + ofc;
    }
    uint32_t extra;
    (void)cze_wg_scan(xb, &extra);
    /* the block's own tables */
    if (lane == 0 && wave < 3) czf_normalise<USER>(wave, n);
    __syncthreads();
    const uint32_t active = (czf.used[0] >= 2 ? 1u : 0u) | (czf.used[1] >= 2 ? 2u : 0u) | (czf.used[2] >= 2 ? 4u : 0u);
    if (active) czf_build<USER>(1u, active);
    /* the six chains: state after sequence k from the state after k + 1 and the code of k */
    if (t < 6 && (!(t & 1u) || ((active >> (t >> 1)) & 1u))) {
        const uint32_t tb = t, size = 1u << czf.log[tb];
        const uint8_t* c = code + (tb >> 1) * CZE_MAX_SEQ;
        uint16_t* r = rec + tb * CZE_MAX_SEQ;
        uint32_t s = czf.first[tb][c[n - 1]], bits = 0;
        r[n - 1] = 0;
        for (int k = (int)n - 2; k >= 0; k--) {
            const uint32_t sym = c[k], x = s + size, nb = (x + czf.dnb[tb][sym]) >> 16;
            r[k] = (uint16_t)((x & ((1u << nb) - 1u)) | (nb << 12));
            s = czf.fstate[tb][(int)(x >> nb) + czf.dfs[tb][sym]];
            bits += nb;
        }
        czf.bits[tb] = bits + czf.log[tb]; czf.fin[tb] = s;
    }
    __syncthreads();
    /* modes, header, descriptions */
    if (t == 0) {
        const uint32_t cnt = n < 128 ? 1u : (n < 0x7F00 ? 2u : 3u);
        uint32_t h = cnt + 1, total = extra;
        for (uint32_t f = 0; f < 3; f++) {
            uint32_t mode = 0, best = czf.bits[2 * f];
            if (czf.used[f] == 1 && 8u < best) { mode = 1; best = 8; }
            if (czf.used[f] >= 2 && 8u * czf.desc_len[f] + czf.bits[2 * f + 1] < best) { mode = 2; best = 8u * czf.desc_len[f] + czf.bits[2 * f + 1]; }
            czf.mode[f] = mode;
            h += mode == 1 ? 1u : (mode == 2 ? czf.desc_len[f] : 0u);
            total += mode == 0 ? czf.bits[2 * f] : (mode == 2 ? czf.bits[2 * f + 1] : 0u);
        }
        const uint32_t fail = h + (total >> 3) + 1 > lim;
        czf.hdr = h; czf.total = total; czf.fail = fail;
        if (!fail) {
            uint32_t p = 0;
            if (cnt == 1) out[p++] = (uint8_t)n;
            else if (cnt == 2) { out[p++] = (uint8_t)((n >> 8) + 128); out[p++] = (uint8_t)n; }
            else { out[p++] = 0xFF; out[p++] = (uint8_t)(n - 0x7F00); out[p++] = (uint8_t)((n - 0x7F00) >> 8); }
            out[p++] = (uint8_t)((czf.mode[CZF_LL] << 6) | (czf.mode[CZF_OF] << 4) | (czf.mode[CZF_ML] << 2));
            for (uint32_t f = 0; f < 3; f++) {
                if (czf.mode[f] == 1) out[p++] = (uint8_t)czf.only[f];
                else if (czf.mode[f] == 2) for (uint32_t i = 0; i < czf.desc_len[f]; i++) out[p++] = czf.desc[f][i];
            }
        }
    }
    __syncthreads();
    if (czf.fail) return lim + 1;
    const uint32_t h = czf.hdr, total = czf.total;
    const uint32_t mLL = czf.mode[CZF_LL], mOF = czf.mode[CZF_OF], mML = czf.mode[CZF_ML];
    const uint16_t* rLL = rec + (2 * CZF_LL + (mLL == 2)) * CZE_MAX_SEQ;
    const uint16_t* rOF = rec + (2 * CZF_OF + (mOF == 2)) * CZE_MAX_SEQ;
    const uint16_t* rML = rec + (2 * CZF_ML + (mML == 2)) * CZE_MAX_SEQ;
    /* the bit stream, last sequence first: per sequence the OF, ML and LL state bits, then the LL, ML and OF extra bits */
    for (uint32_t k = t; k < (total + 32u) / 32u + 2u; k += CZE_THREADS) W[k] = 0;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += CZE_THREADS) {
        const uint32_t j = t0 + t, live = j < n, k = live ? n - 1 - j : 0;
        uint64_t a = 0, b = 0; uint32_t na = 0, nb = 0;
        if (live) {
            const CzeSeq q = sq[k];
            const uint32_t ll = (k + 1 < n ? sq[k + 1].lpos : nlit) - q.lpos;
            const uint32_t llc = code[CZF_LL * CZE_MAX_SEQ + k], ofc = code[CZF_OF * CZE_MAX_SEQ + k], mlc = code[CZF_ML * CZE_MAX_SEQ + k];
            if (mOF != 1) { const uint32_t r = rOF[k]; a |= (uint64_t)(r & 0xFFFu) << na; na += r >> 12; }
            if (mML != 1) { const uint32_t r = rML[k]; a |= (uint64_t)(r & 0xFFFu) << na; na += r >> 12; }
            if (mLL != 1) { const uint32_t r = rLL[k]; a |= (uint64_t)(r & 0xFFFu) << na; na += r >> 12; }
            a |= (uint64_t)(ll - CZ_LL_BASE[llc]) << na; na += CZ_LL_BITS[llc];
            b = q.ml - CZ_ML_BASE[mlc]; nb = CZ_ML_BITS[mlc];
            b |= (uint64_t)(q.off - (1u << ofc)) << nb; nb += ofc;
        }
        uint32_t tot;
        const uint32_t o = base + cze_wg_scan(na + nb, &tot);
        czf_or(W, o, a, na); czf_or(W, o + na, b, nb);
        base += tot;
    }
    __syncthreads();
    if (t == 0) {                                                       /* the initial states (ML, OF, LL) and the closing bit */
        uint32_t o = base;
        if (mML != 1) { const uint32_t tb = 2 * CZF_ML + (mML == 2); czf_or(W, o, czf.fin[tb], czf.log[tb]); o += czf.log[tb]; }
        if (mOF != 1) { const uint32_t tb = 2 * CZF_OF + (mOF == 2); czf_or(W, o, czf.fin[tb], czf.log[tb]); o += czf.log[tb]; }
        if (mLL != 1) { const uint32_t tb = 2 * CZF_LL + (mLL == 2); czf_or(W, o, czf.fin[tb], czf.log[tb]); o += czf.log[tb]; }
        czf_or(W, o, 1, 1);
    }
    __syncthreads();
    const uint32_t len = (total >> 3) + 1;
    const uint8_t* src = (const uint8_t*)W;
    for (uint32_t i = t; i < len; i += CZE_THREADS) out[h + i] = src[i];
    __syncthreads();
    return h + len;
}

/* One block [b0, b1) of the input into st: the 3-byte header, then the body, Raw, RLE or Compressed, whichever is smallest.  The
   pipeline of cz_compress_frames_kernel, step for step, up to the sequences section, on the workgroup's table (cze.htab) and offset
   history (cze.rep), which a block that is not written Compressed leaves as it found it.  Returns 3 + the body's length (every
   thread).  Always inlined: as a function of its own, called from two kernels and touching LDS, it made the compiler number the
   kernels for an LDS address table, which renumbered — and re-allocated registers in — the decode kernels of the same module. */
__device__ static __forceinline__ uint32_t czf_block(const uint8_t* in, uint32_t b0, uint32_t b1, uint32_t last, uint8_t* st, uint8_t* lit, CzeSeq* seqs,
                                     uint32_t* hufw, uint8_t* fscr) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t bsize = b1 - b0;
    uint8_t* blk = st + 3;
    if (t == 0) cze.rle = bsize > 0;
    __syncthreads();
    for (uint32_t k = t; k < bsize; k += CZE_THREADS) if (in[b0 + k] != in[b0]) cze.rle = 0;
    __syncthreads();
    const uint32_t rle = cze.rle;
    uint32_t btype = 0, csize = 0;                                      /* 0 Raw, 1 RLE, 2 Compressed */
    if (rle) btype = 1;
    else if (bsize >= 16) {
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
        const uint32_t nsl = cze.nseqlit;
        for (uint32_t s = wave; s <= nseq; s += CZE_WAVES) {
            uint32_t src, dst, n;
            if (s < nseq) { const CzeSeq q = seqs[s]; dst = q.lpos; n = (s + 1 < nseq ? seqs[s + 1].lpos : nsl) - dst; src = b0 + q.mstart - n; }
            else { dst = nsl; n = nlit - nsl; src = b1 - n; }
            for (uint32_t k = lane; k < n; k += 64) lit[dst + k] = in[src + k];
        }
        __syncthreads();
        /* repeat offsets, forward.  A history of (0, 0, 0) equals no offset: the first sequence then comes out explicit. */
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
        const uint32_t lsz = cze_literals<false, 2>(lit, nlit, blk, hufw, nullptr, 0u, nullptr);
        if (lsz < bsize) {
            __syncthreads();                                            /* the literals' streams have left hufw */
            csize = lsz + czf_sequences(seqs, nseq, nsl, blk + lsz, bsize - lsz, hufw, fscr);
            if (csize < bsize) btype = 2;
        }
        if (btype != 2) {                                               /* the decoder will not see these sequences */
            __syncthreads();
            if (t == 0) { cze.rep[0] = r0; cze.rep[1] = r1; cze.rep[2] = r2; }
        }
    }
    const uint32_t body = btype == 0 ? bsize : (btype == 1 ? 1u : csize);
    const uint32_t bh = last | (btype << 1) | ((btype == 2 ? csize : bsize) << 3);
    if (t == 0) { st[0] = (uint8_t)bh; st[1] = (uint8_t)(bh >> 8); st[2] = (uint8_t)(bh >> 16); }
    if (btype != 2) cze_copy(blk, in + b0, body);
    __syncthreads();
    return 3 + body;
}

/* cz_compress_frames_kernel with CZ_COMPRESS_FSE_TABLES: a workgroup per frame from the work counter; every block is built in the
   workgroup's scratch and copied out when it fits out_cap */
__global__ void __launch_bounds__(CZE_THREADS) cz_compress_frames_fse_kernel(cz_enc_args a) {
    const uint32_t t = threadIdx.x, wave = t >> 6;
    czf_predefined();
    uint8_t* scr = a.scratch + (uint64_t)blockIdx.x * a.scratch_stride;
    uint8_t* lit = scr + CZE_SCR_LIT;
    CzeSeq* seqs = (CzeSeq*)(scr + CZE_SCR_SEQ);
    uint32_t* hufw = (uint32_t*)(scr + CZE_SCR_HUF);
    uint8_t* stage = scr + CZE_SCR_BLK;
    uint8_t* fscr = scr + CZE_SCRATCH_BYTES;
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
        const uint32_t cks = a.flags & CZ_COMPRESS_CHECKSUM, flags = cks | CZ_COMPRESS_FSE_TABLES;
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
        hdr[hl++] = (uint8_t)((fcs_flag << 6) | (single << 5) | (cks ? 4u : 0u));
        if (!single) hdr[hl++] = (uint8_t)((20 - 10) << 3);            /* Window_Descriptor: 1 MiB */
        if (fcs_flag == 0) hdr[hl++] = (uint8_t)len;
        else if (fcs_flag == 1) { hdr[hl++] = (uint8_t)(len - 256); hdr[hl++] = (uint8_t)((len - 256) >> 8); }
        else for (int i = 0; i < 4; i++) hdr[hl++] = (uint8_t)(len >> (8 * i));
        int status = CZ_OK; uint64_t pos = 0; uint32_t nblocks = 0, done = 0;
        if (hl <= cap) { for (uint32_t i = t; i < hl; i += CZE_THREADS) out[i] = hdr[i]; pos = hl; }
        else status = CZ_E_OUTPUT_TOO_SMALL;
        __syncthreads();
        for (uint32_t b0 = 0; status == CZ_OK && (b0 < len || (len == 0 && nblocks == 0));) {
            const uint32_t b1 = len - b0 < CZE_BLOCK ? len : b0 + CZE_BLOCK;
            const uint32_t sz = czf_block(in, b0, b1, b1 == len, stage, lit, seqs, hufw, fscr);
            if (pos + sz > cap) { status = CZ_E_OUTPUT_TOO_SMALL; break; }
            cze_copy(out + pos, stage, sz);
            pos += sz; nblocks++; done = b1;
            b0 = b1;
            __syncthreads();
        }
        uint32_t sum = 0;
        if (status == CZ_OK && cks) {
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

/* cz_compress_segments_kernel with CZ_COMPRESS_FSE_TABLES: the same units from the same plan, the same chain word and waits
   (czstd_encsplit.hip has the argument for progress); only the per-block function differs */
__global__ void __launch_bounds__(CZE_THREADS) cz_compress_segments_fse_kernel(cz_encsplit_args sa) {
    const cz_enc_args& a = sa.a;
    const uint32_t t = threadIdx.x, wave = t >> 6;
    const unsigned long long total = sa.unit_base[a.n];
    if (t == 0) czs.unit = atomicAdd(sa.counter, 1ull);
    __syncthreads();
    if (czs.unit >= total) return;                                      /* a workgroup without work */
    czf_predefined();
    uint8_t* scr = a.scratch + (uint64_t)blockIdx.x * a.scratch_stride;
    uint8_t* lit = scr + CZE_SCR_LIT;
    CzeSeq* seqs = (CzeSeq*)(scr + CZE_SCR_SEQ);
    uint32_t* hufw = (uint32_t*)(scr + CZE_SCR_HUF);
    uint8_t* stage = scr + CZE_SCR_STAGE;
    uint8_t* fscr = scr + CZE_SPLIT_SCRATCH_BYTES;
    for (uint32_t claimed = 1;; claimed = 0) {
        if (!claimed) { __syncthreads(); if (t == 0) czs.unit = atomicAdd(sa.counter, 1ull); }
        __syncthreads();
        const unsigned long long unit = czs.unit;
        if (unit >= total) break;
        /* the frame of the unit: the last f with unit_base[f] <= unit; a closed frame's later segments have nothing to do */
        if (t == 0) {
            uint32_t lo = 0, hi = a.n - 1;
            while (lo < hi) { const uint32_t mid = lo + (hi - lo + 1) / 2; if (sa.unit_base[mid] <= unit) lo = mid; else hi = mid - 1; }
            czs.frame = lo; czs.local = (uint32_t)(unit - sa.unit_base[lo]);
            czs.skip = CZE_CH_STATE(CZ_LD_AGENT(&sa.fstate[2 * (uint64_t)lo])) >= CZE_CH_TOO_SMALL;
        }
        __syncthreads();
        const uint32_t f = czs.frame, local = czs.local;
        if (czs.skip) continue;
        const uint8_t* in = a.in_base + a.in_off[f];
        const uint64_t len64 = a.in_len[f];
        uint8_t* out = a.out_base + a.out_off[f];
        const uint64_t cap = a.out_cap[f];
        cz_compress_result* res = a.results + f;
        unsigned long long* chain = &sa.fstate[2 * (uint64_t)f];
        const uint32_t cks = a.flags & CZ_COMPRESS_CHECKSUM;
        if (len64 >= 0xFFF00000ull) {                                   /* positions are 32-bit */
            if (t == 0) { res->status = CZ_E_INVALID_ARG; res->blocks = 0; res->bytes_read = 0; res->bytes_written = 0; res->checksum = 0; res->flags = cks | CZ_COMPRESS_FSE_TABLES; }
            continue;
        }
        const uint32_t len = (uint32_t)len64, split = len > CZE_SEG;
        const uint32_t flags = cks | CZ_COMPRESS_FSE_TABLES | (split ? CZ_COMPRESS_SPLIT : 0u);
        if (split && cks && local == 0) {                               /* the checksum unit: one wave, off the chain's path */
            if (wave == 0) { const uint64_t x = cze_xxh64(in, len); if (t == 0) CZ_ST_AGENT(chain + 1, (1ull << 32) | (uint32_t)x); }
            continue;
        }
        const uint32_t seg = local - (split && cks ? 1u : 0u);
        const uint32_t s0 = seg * CZE_SEG, s1 = len - s0 < CZE_SEG ? len : s0 + CZE_SEG;
        const uint32_t nb = len == 0 ? 1u : (s1 - s0 + CZE_BLOCK - 1) / CZE_BLOCK, blocks_before = seg * CZE_SEG_BLOCKS;
        const uint32_t last_seg = s1 == len;
        /* the table: empty, then for a later segment the overlap in front of it */
        for (uint32_t k = t; k < (1u << CZE_HASH_LOG); k += CZE_THREADS) cze.htab[k] = 0;
        if (t == 0) { cze.rep[0] = seg ? 0u : 1u; cze.rep[1] = seg ? 0u : 4u; cze.rep[2] = seg ? 0u : 8u; }
        __syncthreads();
        if (seg) {
            for (uint32_t p = (s0 > CZE_OVERLAP ? s0 - CZE_OVERLAP : 0u) + t; p < s0; p += CZE_THREADS)
                if (p + 4 <= len) atomicMax(&cze.htab[cze_hash(cze_ld4(in + p))], p + 1);
            __syncthreads();
        }
        /* the blocks, staged */
        uint32_t staged = 0;
        for (uint32_t j = 0; j < nb; j++) {
            const uint32_t b0 = s0 + j * CZE_BLOCK, b1 = s1 - b0 < CZE_BLOCK ? s1 : b0 + CZE_BLOCK;
            const uint32_t sz = czf_block(in, b0, b1, b1 == len, stage + staged, lit, seqs, hufw, fscr);
            if (t == 0) czs.bsz[j] = sz;
            staged += sz;
        }
        /* frame header (segment 0) */
        const uint32_t single = len <= (1u << 20);
        uint8_t hdr[14]; uint32_t hl = 0;
        hdr[hl++] = 0x28; hdr[hl++] = 0xB5; hdr[hl++] = 0x2F; hdr[hl++] = 0xFD;
        const uint32_t fcs_flag = single && len < 256 ? 0u : (len >= 256 && len < 65536 + 256 ? 1u : 2u);
        hdr[hl++] = (uint8_t)((fcs_flag << 6) | (single << 5) | (cks ? 4u : 0u));
        if (!single) hdr[hl++] = (uint8_t)((20 - 10) << 3);            /* Window_Descriptor: 1 MiB */
        if (fcs_flag == 0) hdr[hl++] = (uint8_t)len;
        else if (fcs_flag == 1) { hdr[hl++] = (uint8_t)(len - 256); hdr[hl++] = (uint8_t)((len - 256) >> 8); }
        else for (int i = 0; i < 4; i++) hdr[hl++] = (uint8_t)(len >> (8 * i));
        /* lane 0: where the segment goes (act 0: nowhere, the frame is closed; 1: placed; else the state that closes the frame
           here), how many of its blocks fit, and the word for the successors — published before the copy */
        __syncthreads();
        if (t == 0) {
            unsigned long long w = 0; uint64_t pos = 0; uint32_t act = 1, nfit = 0;
            if (seg == 0) { if (hl <= cap) pos = hl; else act = (uint32_t)CZE_CH_TOO_SMALL; }
            else if (!cze_wait_chain(chain, blocks_before, &w)) act = (uint32_t)CZE_CH_EXPIRED;
            else if (CZE_CH_STATE(w) >= CZE_CH_TOO_SMALL) act = 0;
            else pos = CZE_CH_POS(w);
            uint64_t end = pos;
            if (act == 1) {
                while (nfit < nb && end + czs.bsz[nfit] <= cap) { end += czs.bsz[nfit]; nfit++; }
                if (nfit < nb) act = (uint32_t)CZE_CH_TOO_SMALL;
                else if (!last_seg) (void)atomicMax(chain, CZE_CH_WORD(0, blocks_before + nb, end));
            }
            uint32_t first = 0;
            if (act >= CZE_CH_TOO_SMALL) first = CZE_CH_STATE(atomicMax(chain, CZE_CH_WORD(act, blocks_before + nfit, end))) < CZE_CH_TOO_SMALL;
            czs.word = CZE_CH_WORD(0, 0, pos); czs.act = act; czs.nfit = nfit; czs.first = first;
        }
        __syncthreads();
        const uint32_t act = czs.act, nfit = czs.nfit;
        uint64_t pos = CZE_CH_POS(czs.word);
        if (act == 0) continue;
        if (act == CZE_CH_EXPIRED) {                                    /* where the predecessors stand is not known */
            if (t == 0 && czs.first) { res->status = CZ_E_WAIT_EXPIRED; res->blocks = 0; res->bytes_read = 0; res->bytes_written = 0; res->checksum = 0; res->flags = flags; }
            continue;
        }
        uint32_t fit_bytes = 0;
        for (uint32_t j = 0; j < nfit; j++) fit_bytes += czs.bsz[j];
        if (seg == 0 && hl <= cap) for (uint32_t i = t; i < hl; i += CZE_THREADS) out[i] = hdr[i];
        cze_copy(out + pos, stage, fit_bytes);
        pos += fit_bytes;
        __syncthreads();
        if (act == CZE_CH_TOO_SMALL) {
            if (t == 0 && czs.first) {
                res->status = CZ_E_OUTPUT_TOO_SMALL; res->blocks = blocks_before + nfit; res->bytes_read = (uint64_t)(blocks_before + nfit) * CZE_BLOCK;
                res->bytes_written = pos; res->checksum = 0; res->flags = flags;
            }
            continue;
        }
        if (!last_seg) continue;
        /* the last segment: the checksum (a split frame's comes from its checksum unit), then the result record */
        int status = CZ_OK; uint32_t sum = 0;
        if (cks) {
            if (!split) { if (wave == 0) { const uint64_t x = cze_xxh64(in, len); if (t == 0) czs.sum = (uint32_t)x; } }
            else if (t == 0) {
                /* XXH64 is serial over the input: the bound grows with it (64 bytes per poll) */
                const uint32_t bound = CZE_WAIT_POLLS + (len >> 6);
                unsigned long long w = 0;
                for (uint32_t polls = 0;; polls++) {
                    w = CZ_LD_AGENT(chain + 1);
                    if (w >> 32) break;
                    if (polls >= bound) break;
                    __builtin_amdgcn_s_sleep(64);
                }
                czs.sum = (uint32_t)w;
                czs.nfit = (uint32_t)(w >> 32);                         /* 0: the wait ran into its bound */
            }
            __syncthreads();
            sum = czs.sum;
            if (split && !czs.nfit) {
                if (t == 0) {
                    (void)atomicMax(chain, CZE_CH_WORD(CZE_CH_EXPIRED, 0, 0));
                    res->status = CZ_E_WAIT_EXPIRED; res->blocks = 0; res->bytes_read = 0; res->bytes_written = 0; res->checksum = 0; res->flags = flags;
                }
                continue;
            }
            if (pos + 4 > cap) status = CZ_E_OUTPUT_TOO_SMALL;
            else { if (t < 4) out[pos + t] = (uint8_t)(sum >> (8 * t)); pos += 4; }
        }
        if (t == 0) {
            res->status = status; res->blocks = blocks_before + nb; res->bytes_read = len; res->bytes_written = pos;
            res->checksum = sum; res->flags = flags;
        }
    }
}
