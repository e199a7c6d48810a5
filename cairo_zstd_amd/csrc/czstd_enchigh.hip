/*
 * czstd_enchigh.hip — CZ_COMPRESS_HIGH: the high-ratio level.
 *
 * The frames are those of CZ_COMPRESS_FSE_TABLES (czstd_encfse.hip) in everything but the choice of sequences: the same header,
 * blocks, literals (cze_literals) and sequences sections (czf_sequences).  What differs is how a block's sequences are found:
 *
 *     match pass    every position of a chunk keeps the better of three candidates: the nearest position with the same 4-byte hash
 *                   among the 64 before it in the chunk, the entry of the 4-byte table (cze.htab) and the entry of a second table
 *                   keyed by the hash of 8 bytes (czh.htab8), which keeps a long match when a nearer short one has taken the 4-byte
 *                   entry.  The longer candidate wins, the nearer one on equal (capped) length.  Both tables are read before the
 *                   chunk's inserts and every insert is an atomicMax, so the bytes do not depend on timing.
 *     parse         wave 0, serial over the chunk's matches.  At a position with a table match it measures the live offset history
 *                   there (one 64-lane compare and a ballot per entry) and takes a repeat match when it is at most CZH_REP_BONUS
 *                   bytes shorter than the table match.  A match below CZE_CAP is lazy: it looks at the kept table matches at
 *                   p + 1 and p + 2 and at the history at p + 1, and moves on when one of them is longer by more than the literals
 *                   it costs (a repeat match counts CZH_REP_BONUS longer).  It never looks past the end of the chunk in hand.
 *     offsets       the parse carries the history and writes Offset_Values itself, all six repeat cases of RFC 8878 §3.1.1.5; an
 *                   offset that the history holds in a usable place is never written in full.
 *
 * Included behind czstd_encfse.hip.  The helpers it shares are instantiated with a USER of this file's own (cze_match and
 * cze_literals 4, czf_predefined and czf_sequences 1) and czh_block is always inlined, so the kernels in front of this file compile
 * as they did without it.
 */
#define CZH_REP_BONUS 2u        /* a repeat match may be this much shorter than a table match and still win */
#define CZH_HASH8_LOG 14
#define CZE_HIGH_SCRATCH_BYTES CZE_FSE_SCRATCH_BYTES

struct CzhShared {
    uint32_t htab8[1u << CZH_HASH8_LOG];                                /* as cze.htab, keyed by the hash of 8 bytes */
};
__shared__ CzhShared czh;

__device__ static inline uint32_t czh_hash8(const uint8_t* p) {
    uint64_t v; __builtin_memcpy(&v, p, 8);
    return (uint32_t)((v * 0xCF1BBCDCB7A56463ull) >> (64 - CZH_HASH8_LOG));
}

/* wave 0, every lane: the length of the match at p with offset `off` (1 <= off <= p), known to hold for `have` bytes, up to lim */
__device__ static inline uint32_t czh_extend(const uint8_t* in, uint32_t p, uint32_t off, uint32_t have, uint32_t lim, uint32_t lane) {
    uint32_t len = have;
    for (;;) {
        const uint32_t r = p + len + lane;
        const uint64_t bad = __ballot(r >= lim || in[r] != in[r - off]);
        if (!bad) { len += 64; continue; }
        return len + (uint32_t)__ffsll((long long)bad) - 1;
    }
}

/* wave 0, every lane: the best repeat match at p after ll literals under the history (h0, h1, h2) — the longest, the earlier
   entry on a tie; *roff its offset.  0 when none reaches 4 bytes. */
__device__ static inline uint32_t czh_rep(const uint8_t* in, uint32_t p, uint32_t ll, uint32_t h0, uint32_t h1, uint32_t h2, uint32_t lim,
                                          uint32_t lane, uint32_t* roff) {
    const uint32_t c[3] = { ll ? h0 : h1, ll ? h1 : h2, ll ? h2 : h0 - 1u };
    uint32_t best = 0, boff = 0;
    for (uint32_t i = 0; i < 3; i++) {
        if (c[i] == 0 || c[i] > p) continue;
        const uint32_t m = czh_extend(in, p, c[i], 0u, lim, lane);
        if (m >= 4 && m > best) { best = m; boff = c[i]; }
    }
    *roff = boff;
    return best;
}

/* czf_block with the match pass, the parse and the repeat offsets of this level.  Always inlined, as czf_block is.  MU and FU are the
   USER of the helpers it calls (cze_match and cze_literals; czf_sequences): a second kernel around it (czstd_enchighsplit.hip) takes
   values of its own, so that the helpers of the kernel below keep their one caller. */
template <int MU = 4, int FU = 1>
__device__ static __forceinline__ uint32_t czh_block(const uint8_t* in, uint32_t b0, uint32_t b1, uint32_t last, uint8_t* st, uint8_t* lit, CzeSeq* seqs,
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
        const uint32_t r0 = cze.rep[0], r1 = cze.rep[1], r2 = cze.rep[2];
        uint32_t pp = b0, lit_start = b0, nseq = 0, nlit = 0;
        uint32_t h0 = r0, h1 = r1, h2 = r2;                             /* the history as the parse goes (wave 0) */
        for (uint32_t c0 = b0; c0 < b1; c0 += CZE_CHUNK) {
            const uint32_t p = c0 + t, valid = p + 4 <= b1, valid8 = p + 8 <= b1;
            const uint32_t h = valid ? cze_hash(cze_ld4(in + p)) : 0xFFFFFFFFu;
            const uint32_t h8 = valid8 ? czh_hash8(in + p) : 0u;
            cze.chash[t] = h;
            const uint32_t old = valid ? cze.htab[h] : 0, old8 = valid8 ? czh.htab8[h8] : 0;
            __syncthreads();
            uint32_t mlen = 0, moff = 0;
            if (valid) {
                const uint32_t lo = t > CZE_BACK ? t - CZE_BACK : 0;
                for (int j = (int)t - 1; j >= (int)lo; j--) if (cze.chash[j] == h) {
                    const uint32_t m = cze_match<MU>(in, p, c0 + (uint32_t)j, b1);
                    if (m >= 4) { mlen = m; moff = t - (uint32_t)j; }
                    break;
                }
                if (old && p - (old - 1) <= CZE_WINDOW) {               /* further than any in-chunk candidate: longer only */
                    const uint32_t m = cze_match<MU>(in, p, old - 1, b1);
                    if (m >= 4 && m > mlen) { mlen = m; moff = p - (old - 1); }
                }
                if (old8 && old8 != old && p - (old8 - 1) <= CZE_WINDOW) {
                    const uint32_t m = cze_match<MU>(in, p, old8 - 1, b1), o = p - (old8 - 1);
                    if (m >= 4 && (m > mlen || (m == mlen && o < moff))) { mlen = m; moff = o; }
                }
                atomicMax(&cze.htab[h], p + 1);
                if (valid8) atomicMax(&czh.htab8[h8], p + 1);
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
                    for (;;) {                                          /* at pp: a table match, or a repeat match seen from pp - 1 */
                        const uint32_t ll = pp - lit_start;
                        uint32_t ml = cze.cmlen[pp - c0], off = cze.cmoff[pp - c0], bonus = 0;
                        if (ml >= CZE_CAP) ml = czh_extend(in, pp, off, ml, b1, lane);
                        uint32_t roff;
                        const uint32_t rl = czh_rep(in, pp, ll, h0, h1, h2, b1, lane, &roff);
                        if (rl && rl + CZH_REP_BONUS >= ml) { ml = rl; off = roff; bonus = CZH_REP_BONUS; }
                        if (ml < CZE_CAP && pp + 1 < cend) {            /* lazy, inside the chunk */
                            const uint32_t gain = ml + bonus;
                            uint32_t roff1;
                            const uint32_t rl1 = czh_rep(in, pp + 1, ll + 1, h0, h1, h2, b1, lane, &roff1);
                            const uint32_t m1 = cze.cmlen[pp + 1 - c0];
                            const uint32_t g1 = rl1 && rl1 + CZH_REP_BONUS > m1 ? rl1 + CZH_REP_BONUS : m1;
                            if (g1 > gain + 1) { pp += 1; continue; }
                            if (pp + 2 < cend && cze.cmlen[pp + 2 - c0] > gain + 2) { pp += 2; continue; }
                        }
                        /* the Offset_Value and the history behind it */
                        uint32_t ofv;
                        if (ll) {
                            if (off == h0) ofv = 1;
                            else if (off == h1) { ofv = 2; h1 = h0; h0 = off; }
                            else { ofv = off == h2 ? 3u : off + 3; h2 = h1; h1 = h0; h0 = off; }
                        } else {
                            if (off == h1) { ofv = 1; h1 = h0; h0 = off; }
                            else { ofv = off == h2 ? 2u : (off + 1 == h0 ? 3u : off + 3); h2 = h1; h1 = h0; h0 = off; }
                        }
                        if (lane == 0) { CzeSeq s; s.mstart = pp - b0; s.ml = ml; s.off = ofv; s.lpos = nlit; seqs[nseq] = s; }
                        nlit += ll; nseq++;
                        pp += ml; lit_start = pp;
                        break;
                    }
                }
            }
        }
        if (t == 0) { cze.nseq = nseq; cze.nseqlit = nlit; cze.nlit = nlit + (b1 - lit_start); cze.rep[0] = h0; cze.rep[1] = h1; cze.rep[2] = h2; }
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
        const uint32_t lsz = cze_literals<false, MU>(lit, nlit, blk, hufw, nullptr, 0u, nullptr);
        if (lsz < bsize) {
            __syncthreads();                                            /* the literals' streams have left hufw */
            csize = lsz + czf_sequences<FU>(seqs, nseq, nsl, blk + lsz, bsize - lsz, hufw, fscr);
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

/* cz_compress_frames_fse_kernel around czh_block: a workgroup per frame from the work counter, both tables live for the frame */
__global__ void __launch_bounds__(CZE_THREADS) cz_compress_frames_high_kernel(cz_enc_args a) {
    const uint32_t t = threadIdx.x, wave = t >> 6;
    czf_predefined<1>();
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
        const uint32_t cks = a.flags & CZ_COMPRESS_CHECKSUM, flags = cks | CZ_COMPRESS_HIGH;
        if (len64 >= 0xFFF00000ull) {                                   /* positions are 32-bit */
            if (t == 0) { res->status = CZ_E_INVALID_ARG; res->blocks = 0; res->bytes_read = 0; res->bytes_written = 0; res->checksum = 0; res->flags = flags; }
            continue;
        }
        const uint32_t len = (uint32_t)len64;
        for (uint32_t k = t; k < (1u << CZE_HASH_LOG); k += CZE_THREADS) cze.htab[k] = 0;
        for (uint32_t k = t; k < (1u << CZH_HASH8_LOG); k += CZE_THREADS) czh.htab8[k] = 0;
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
            const uint32_t sz = czh_block(in, b0, b1, b1 == len, stage, lit, seqs, hufw, fscr);
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
