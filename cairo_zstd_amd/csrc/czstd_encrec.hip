/*
 * czstd_encrec.hip — CZ_COMPRESS_RECORDS: the records level, one wave per record, with or without dictionaries.
 *
 * cz_compress_records_kernel / cz_compress_records_dict_kernel: persistent 256-thread workgroups whose four waves never meet after
 * the Predefined tables are built.  Every wave claims its next record from the work counter itself and writes the whole frame of
 * that record with wave-level synchronisation only: the header, ONE block in its own scratch slot, the copy out, the checksum and
 * the result record.  A record is at most CZR_MAX = 32 KiB.
 *
 * Without a dictionary the block is czq_block of czstd_encfast.hip, so the frame is the CZ_COMPRESS_FAST frame of the same input.
 * With a dictionary the match pass tries, per position and in this order, the nearest earlier position of its 64-position chunk
 * with the same 12-bit hash, the wave's own table (2^12 x 16 bit, record-local) and the dictionary image's table where it lies in
 * HBM (CzeDict::htab, 2^14 x 32 bit; the 12-bit hash is the 14-bit one >> 2, so one hash serves both).  Positions are the virtual
 * ones of §10.1 and a match may run across the content's end into the input.  The literals may be Treeless with the dictionary's
 * code and each of LL / OF / ML is in Repeat_Mode with the dictionary's table when that has a state for every code of the block;
 * code and tables are read from the image in HBM.  Offset_Value 1 only for the offset of the sequence before it in the block: the
 * dictionary's three repeat offsets are never referred to.
 *
 * The frame bytes depend on the input, the dictionary and the flags alone.  Included behind czstd_encfast.hip; uses its wave-level
 * helpers and its LDS (CzqShared) as they are, so the kernels in front of it compile as they did without it.
 */
#define CZR_MAX CZQ_SUB
/* a wave's slot: the fast level's slot (czq_block works in it), then the sequence records of the dictionary path */
#define CZR_SCR_DSEQ CZQ_SLOT_BYTES
#define CZR_SLOT_BYTES (CZR_SCR_DSEQ + CZQ_MAX_SEQ * 12u)
#define CZE_RECORDS_SCRATCH_BYTES (CZE_WAVES * CZR_SLOT_BYTES)

/* one sequence of a record with a dictionary: as CzqSeq, with an offset that reaches into the content */
struct CzrSeq { uint32_t off; uint16_t mstart, ml, lpos, pad; };

__device__ static inline uint32_t czr_offset_value(const CzrSeq* sq, uint32_t k, uint32_t ll) {
    const uint32_t off = sq[k].off;
    return k > 0 && ll > 0 && sq[k - 1].off == off ? 1u : off + 3u;
}

/* the wave: the sequences section of n sequences at out[0, lim) as czq_sequences writes it, but each of LL / OF / ML (bit 0 / 1 / 2
   of the mode mask) in Repeat_Mode with the table of img when that has a state for every code of the block, else Predefined (the
   workgroup's tables in LDS).  Returns its length, or lim + 1 when it does not fit (every lane). */
__device__ static uint32_t czr_sequences(CzqWave& S, const CzeDict* img, const CzrSeq* sq, uint32_t n, uint32_t nlit, uint8_t* out, uint32_t lim,
                                         uint32_t* W, uint8_t* code, uint16_t* rec) {
    const uint32_t lane = threadIdx.x & 63u;
    if (n == 0) { if (lane == 0 && lim >= 1) out[0] = 0; return lim >= 1 ? 1u : lim + 1; }
    uint32_t xb = 0, lack = 0;
    for (uint32_t k = lane; k < n; k += 64) {
        const uint32_t ll = (k + 1 < n ? sq[k + 1].lpos : nlit) - sq[k].lpos;
        const uint32_t llc = cze_ll_code(ll), mlc = cze_ml_code(sq[k].ml), ofc = cze_hb(czr_offset_value(sq, k, ll));
        code[0 * CZQ_MAX_SEQ + k] = (uint8_t)llc; code[1 * CZQ_MAX_SEQ + k] = (uint8_t)ofc; code[2 * CZQ_MAX_SEQ + k] = (uint8_t)mlc;
        xb += CZ_LL_BITS[llc] + CZ_ML_BITS[mlc] + ofc;
        lack |= (img->ffirst[0][llc] == 0xFFFFu ? 1u : 0u) | (img->ffirst[1][ofc] == 0xFFFFu ? 2u : 0u) | (img->ffirst[2][mlc] == 0xFFFFu ? 4u : 0u);
    }
    const uint32_t rm = (__ballot((int)(lack & 1u)) ? 0u : 1u) | (__ballot((int)(lack & 2u)) ? 0u : 2u) | (__ballot((int)(lack & 4u)) ? 0u : 4u);
    uint32_t extra;
    (void)czq_scan(xb, &extra);
    cz_wave_sync();
    /* the three chains side by side: state after sequence k from the state after k + 1 and the code of k */
    if (lane < 3) {
        const uint32_t tb = lane, rep = (rm >> tb) & 1u, log = rep ? img->flog[tb] : czq_log(tb), size = 1u << log;
        const uint8_t* c = code + tb * CZQ_MAX_SEQ;
        uint16_t* r = rec + tb * CZQ_MAX_SEQ;
        uint32_t s = rep ? img->ffirst[tb][c[n - 1]] : czq.first[tb][c[n - 1]], bits = 0;
        r[n - 1] = 0;
        for (int k = (int)n - 2; k >= 0; k--) {
            const uint32_t sym = c[k], x = s + size, nb = (x + (rep ? img->fdnb[tb][sym] : czq.dnb[tb][sym])) >> 16;
            r[k] = (uint16_t)((x & ((1u << nb) - 1u)) | (nb << 12));
            const int at = (int)(x >> nb) + (rep ? img->fdfs[tb][sym] : czq.dfs[tb][sym]);
            s = rep ? img->fstate[tb][at] : czq.fstate[tb][at];
            bits += nb;
        }
        S.bits[tb] = bits + log; S.fin[tb] = s | (log << 16);
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
        out[p++] = (uint8_t)((rm & 1u ? 3u << 6 : 0u) | (rm & 2u ? 3u << 4 : 0u) | (rm & 4u ? 3u << 2 : 0u));   /* Predefined or Repeat */
    }
    /* the bit stream, last sequence first: per sequence the OF, ML and LL state bits, then the LL, ML and OF extra bits */
    for (uint32_t k = lane; k < (total + 32u) / 32u + 2u; k += 64) W[k] = 0;
    cz_wave_sync();
    uint32_t base = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += 64) {
        const uint32_t j = t0 + lane, live = j < n, k = live ? n - 1 - j : 0;
        uint64_t a = 0, b = 0; uint32_t na = 0, nb = 0;
        if (live) {
            const uint32_t ll = (k + 1 < n ? sq[k + 1].lpos : nlit) - sq[k].lpos, ml = sq[k].ml, ov = czr_offset_value(sq, k, ll);
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
        czq_or(W, o, S.fin[2] & 0xFFFFu, S.fin[2] >> 16); o += S.fin[2] >> 16;
        czq_or(W, o, S.fin[1] & 0xFFFFu, S.fin[1] >> 16); o += S.fin[1] >> 16;
        czq_or(W, o, S.fin[0] & 0xFFFFu, S.fin[0] >> 16); o += S.fin[0] >> 16;
        czq_or(W, o, 1, 1);
    }
    cz_wave_sync();
    const uint32_t len = (total >> 3) + 1;
    const uint8_t* src = (const uint8_t*)W;
    for (uint32_t i = lane; i < len; i += 64) out[h + i] = src[i];
    cz_wave_sync();
    return h + len;
}

/* the wave: the literals section of lit[0, nlit) at out; returns its length (every lane).  czq_literals, then Treeless with the
   code of img when every literal has a code there and the exact size is below what czq_literals wrote (RLE literals stay). */
__device__ static uint32_t czr_literals(CzqWave& S, const CzeDict* img, const uint8_t* lit, uint32_t nlit, uint8_t* out, uint32_t* hufw) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t own = czq_literals<1>(S, lit, nlit, out, hufw);
    if (nlit == 0 || (out[0] & 3u) == 1u) return own;
    const uint32_t four = nlit >= 1024, ns = four ? 4u : 1u, seg = four ? (nlit + 3) / 4 : nlit;
    uint32_t miss = 0, acc[4] = {0, 0, 0, 0};
    for (uint32_t k = lane; k < nlit; k += 64) {
        const uint32_t l = img->hlen[lit[k]], q = k / seg;
        miss |= !l;
        acc[0] += q == 0 ? l : 0u; acc[1] += q == 1 ? l : 0u; acc[2] += q == 2 ? l : 0u; acc[3] += q == 3 ? l : 0u;
    }
    if (__ballot((int)miss)) return own;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < ns; k++) { uint32_t bits; (void)czq_scan(acc[k], &bits); sum += (bits >> 3) + 1; }
    const uint32_t body = (four ? 6u : 0u) + sum;
    const uint32_t hdr = !four ? 3u : (nlit < 16384 && body < 16384 ? 4u : 5u);
    if (hdr + body >= own) return own;
    cz_wave_sync();
    for (uint32_t s = lane; s < 256; s += 64) { S.hlen[s] = img->hlen[s]; S.hcode[s] = img->hcode[s]; }
    cz_wave_sync();
    uint32_t sb[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < ns; k++) {
        const uint32_t s0 = k * seg, s1 = (k + 1) * seg < nlit ? (k + 1) * seg : nlit;
        sb[k] = czq_huf_stream<1>(S, lit, s0, s1, hufw + k * CZQ_HUF_REGION_WORDS);
    }
    if (lane == 0) {
        const uint32_t sf = !four ? 0u : (hdr == 4 ? 2u : 3u);
        const uint32_t nbits = hdr == 3 ? 10u : (hdr == 4 ? 14u : 18u);
        const uint64_t v = 3u | (sf << 2) | ((uint64_t)nlit << 4) | ((uint64_t)body << (4 + nbits));
        for (uint32_t i = 0; i < hdr; i++) out[i] = (uint8_t)(v >> (8 * i));
        if (four) for (uint32_t k = 0; k < 3; k++) { out[hdr + 2 * k] = (uint8_t)sb[k]; out[hdr + 2 * k + 1] = (uint8_t)(sb[k] >> 8); }
    }
    uint32_t at = hdr + (four ? 6u : 0u);
    for (uint32_t k = 0; k < ns; k++) {
        const uint8_t* src = (const uint8_t*)(hufw + k * CZQ_HUF_REGION_WORDS);
        for (uint32_t i = lane; i < sb[k]; i += 64) out[at + i] = src[i];
        at += sb[k];
    }
    cz_wave_sync();
    return hdr + body;
}

/* The record in[0, len), len > 0, after the content dct[0, D) of its dictionary: RLE, Compressed (its body then in blk) or Raw,
   whichever is smallest.  Returns type << 24 | body bytes (every lane).  czq_block with the third candidate and virtual offsets. */
__device__ static __forceinline__ uint32_t czr_dblock(CzqWave& S, const CzeDict* img, const uint8_t* dct, uint32_t D, const uint8_t* in, uint32_t len,
                                                      uint8_t* slot, uint8_t* blk) {
    const uint32_t lane = threadIdx.x & 63u;
    uint8_t* lit = slot + CZQ_SCR_LIT;
    CzrSeq* seqs = (CzrSeq*)(slot + CZR_SCR_DSEQ);
    uint32_t* hufw = (uint32_t*)(slot + CZQ_SCR_HUF);
    /* RLE block? */
    {
        const uint32_t first = in[0], splat = first * 0x01010101u;
        uint32_t rle = 1;
        for (uint32_t k = 0; k < len; k += 256) {
            const uint32_t p = k + 4 * lane;
            uint32_t bad = 0;
            if (p + 4 <= len) bad = cze_ld4(in + p) != splat;
            else for (uint32_t i = p; i < len; i++) bad |= in[i] != first;
            if (__ballot((int)bad)) { rle = 0; break; }
        }
        if (rle) return (1u << 24) | 1u;
    }
    if (len < 16) return len;
    for (uint32_t k = lane; k < (1u << (CZQ_HASH_LOG - 1)); k += 64) S.htab32[k] = 0;
    cz_wave_sync();
    /* matches, chunk by chunk, and the parse of each chunk behind them */
    uint32_t pp = 0, lit_start = 0, nseq = 0, nlit = 0;
    for (uint32_t c0 = 0; c0 < len; c0 += CZQ_CHUNK) {
        const uint32_t p = c0 + lane, valid = p + 4 <= len;
        const uint32_t h14 = valid ? cze_hash(cze_ld4(in + p)) : 0u;
        const uint32_t h = valid ? h14 >> (CZE_HASH_LOG - CZQ_HASH_LOG) : 0xFFFFu;
        S.u.c.chash[lane] = (uint16_t)h;
        const uint32_t old = valid ? S.htab[h] : 0;
        cz_wave_sync();
        uint32_t mlen = 0, moff = 0;
        if (valid) {
            for (int j = (int)lane - 1; j >= 0; j--) if (S.u.c.chash[j] == h) {
                const uint32_t m = cze_match<1>(in, p, c0 + (uint32_t)j, len);
                if (m >= 4) { mlen = m; moff = lane - (uint32_t)j; }
                break;
            }
            if (!mlen && old) {
                const uint32_t m = cze_match<1>(in, p, old - 1, len);
                if (m >= 4) { mlen = m; moff = p - (old - 1); }
            }
            if (!mlen) {
                const uint32_t v = img->htab[h14];                     /* content position + 1 */
                if (v && D + p - (v - 1) <= CZE_WINDOW) {
                    const uint32_t m = cze_dmatch<1>(dct, D, in, p, v - 1, len);
                    if (m >= 4) { mlen = m; moff = D + p - (v - 1); }
                }
            }
        }
        S.u.c.cmlen[lane] = (uint16_t)mlen;
        /* the chunk into the table, highest position wins: whoever finds a lower position than its own in its entry writes again */
        const uint32_t mine = p + 1;
        for (uint32_t pending = valid;;) {
            if (pending) S.htab[h] = (uint16_t)mine;
            cz_wave_sync();
            if (pending && S.htab[h] >= mine) pending = 0;
            if (!__ballot((int)pending)) break;
        }
        const uint32_t cend = c0 + CZQ_CHUNK < len ? c0 + CZQ_CHUNK : len;
        while (pp < cend) {
            const uint32_t q = pp + lane;
            const uint64_t mask = __ballot(q < cend && S.u.c.cmlen[q - c0] >= 4);
            if (!mask) { pp = pp + 64 < cend ? pp + 64 : cend; continue; }
            pp += (uint32_t)__ffsll((long long)mask) - 1;
            uint32_t ml = S.u.c.cmlen[pp - c0];
            const uint32_t off = __shfl(moff, (int)(pp - c0));          /* the offsets stay in registers: they do not fit 16 bits */
            if (ml >= CZE_CAP) {
                for (;;) {
                    const uint32_t r = pp + ml + lane;
                    const uint64_t bad = __ballot(r >= len || in[r] != cze_vb(dct, D, in, D + r - off));
                    if (!bad) { ml += 64; continue; }
                    ml += (uint32_t)__ffsll((long long)bad) - 1;
                    break;
                }
            }
            if (lane == 0) { CzrSeq s; s.off = off; s.mstart = (uint16_t)pp; s.ml = (uint16_t)ml; s.lpos = (uint16_t)nlit; s.pad = 0; seqs[nseq] = s; }
            nlit += pp - lit_start; nseq++;
            pp += ml; lit_start = pp;
        }
    }
    const uint32_t nsl = nlit;                                          /* literals of the sequences; the rest trail the last one */
    nlit += len - lit_start;
    cz_wave_sync();
    /* gather the literals: a lane per sequence (the last: the tail); the wave together on a run above 32 bytes */
    for (uint32_t s0 = 0; s0 <= nseq; s0 += 64) {
        const uint32_t s = s0 + lane;
        uint32_t src = 0, dst = 0, n = 0;
        if (s < nseq) { dst = seqs[s].lpos; n = (s + 1 < nseq ? seqs[s + 1].lpos : nsl) - dst; src = seqs[s].mstart - n; }
        else if (s == nseq) { dst = nsl; n = nlit - nsl; src = len - n; }
        if (n <= 32) for (uint32_t k = 0; k < n; k++) lit[dst + k] = in[src + k];
        for (uint64_t big = __ballot(n > 32); big; big &= big - 1) {
            const int l = __ffsll((long long)big) - 1;
            const uint32_t bn = __shfl(n, l), bsrc = __shfl(src, l), bdst = __shfl(dst, l);
            for (uint32_t k = lane; k < bn; k += 64) lit[bdst + k] = in[bsrc + k];
        }
    }
    cz_wave_sync();
    const uint32_t lsz = czr_literals(S, img, lit, nlit, blk, hufw);
    if (lsz < len) {
        const uint32_t csize = lsz + czr_sequences(S, img, seqs, nseq, nsl, blk + lsz, len - lsz, hufw, slot + CZQ_SCR_CODE, (uint16_t*)(slot + CZQ_SCR_REC));
        if (csize < len) return (2u << 24) | csize;
    }
    return len;
}

/* ------------------------------------------------------------------ the kernels */
/* one more header byte behind the n already in (lo, hi) */
__device__ static inline void czr_push(uint64_t& lo, uint64_t& hi, uint32_t& n, uint32_t byte) {
    if (n < 8) lo |= (uint64_t)(byte & 0xFFu) << (8 * n); else hi |= (uint64_t)(byte & 0xFFu) << (8 * (n - 8));
    n++;
}

template <bool DICT>
__device__ static __forceinline__ void czr_records(cz_enc_args a, cz_enc_dargs d) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    czq_predefined<1>();
    __syncthreads();                                                    /* the last time the four waves meet */
    uint8_t* slot = a.scratch + (uint64_t)blockIdx.x * a.scratch_stride + wave * CZR_SLOT_BYTES;
    uint8_t* blk = slot + CZQ_SCR_BLK;
    CzqWave& S = czq.w[wave];
    const uint32_t cks = a.flags & CZ_COMPRESS_CHECKSUM, flags = cks | CZ_COMPRESS_RECORDS;
    for (;;) {
        cz_wave_sync();
        uint32_t f = 0;
        if (lane == 0) f = atomicAdd(a.work_counter, 1u);
        f = __shfl(f, 0);
        if (f >= a.n) break;
        const uint8_t* in = a.in_base + a.in_off[f];
        const uint64_t len64 = a.in_len[f];
        uint8_t* out = a.out_base + a.out_off[f];
        const uint64_t cap = a.out_cap[f];
        cz_compress_result* res = a.results + f;
        const CzeDict* img = nullptr; const uint8_t* dct = nullptr; uint64_t dlen = 0; uint32_t did = 0, bad_index = 0;
        if (DICT) {
            const uint32_t di = d.dict_index ? d.dict_index[f] : 0u;
            if (di != CZ_COMPRESS_NO_DICT) {
                if (di >= d.ndicts) bad_index = 1;
                else { const cze_dict_entry& e = d.dicts[di]; img = e.img; dct = e.content; dlen = e.content_len; did = e.id; }
            }
        }
        if (len64 > CZR_MAX || len64 + dlen >= 0xFFF00000ull || bad_index) {   /* the level's reach; (virtual) positions are 32-bit */
            if (lane == 0) { res->status = CZ_E_INVALID_ARG; res->blocks = 0; res->bytes_read = 0; res->bytes_written = 0; res->checksum = 0; res->flags = flags; }
            continue;
        }
        const uint32_t len = (uint32_t)len64, D = (uint32_t)dlen;
        /* frame header: Single_Segment, Frame_Content_Size in one byte below 256 and in two from there */
        uint64_t hlo = 0, hhi = 0; uint32_t hl = 0;
        const uint32_t idb = !img || did == 0 || (a.flags & CZ_COMPRESS_NO_DICT_ID) ? 0u : (did < 256 ? 1u : (did < 65536 ? 2u : 4u));
        czr_push(hlo, hhi, hl, 0x28); czr_push(hlo, hhi, hl, 0xB5); czr_push(hlo, hhi, hl, 0x2F); czr_push(hlo, hhi, hl, 0xFD);
        czr_push(hlo, hhi, hl, ((len < 256 ? 0u : 1u) << 6) | (1u << 5) | (cks ? 4u : 0u) | (idb == 4 ? 3u : idb));
        for (uint32_t i = 0; i < idb; i++) czr_push(hlo, hhi, hl, did >> (8 * i));   /* Dictionary_ID: the smallest field that holds it */
        if (len < 256) czr_push(hlo, hhi, hl, len);
        else { czr_push(hlo, hhi, hl, len - 256); czr_push(hlo, hhi, hl, (len - 256) >> 8); }
        int status = CZ_OK; uint64_t pos = 0; uint32_t nblocks = 0, done = 0;
        if (hl <= cap) { if (lane < hl) out[lane] = (uint8_t)(lane < 8 ? hlo >> (8 * lane) : hhi >> (8 * (lane - 8))); pos = hl; }
        else status = CZ_E_OUTPUT_TOO_SMALL;
        if (status == CZ_OK && len == 0) {                              /* one empty last Raw block */
            if (pos + 3 > cap) status = CZ_E_OUTPUT_TOO_SMALL;
            else { if (lane < 3) out[pos + lane] = lane == 0 ? 1 : 0; pos += 3; nblocks = 1; }
        }
        if (status == CZ_OK && len > 0) {
            const uint32_t r = DICT && img ? czr_dblock(S, img, dct, D, in, len, slot, blk) : czq_block<1>(S, in, 0, len, slot, blk);
            const uint32_t btype = r >> 24, body = r & 0xFFFFFFu;
            if (pos + 3 + body > cap) status = CZ_E_OUTPUT_TOO_SMALL;
            else {
                const uint32_t bh = 1u | (btype << 1) | ((btype == 2 ? body : len) << 3);
                if (lane < 3) out[pos + lane] = (uint8_t)(bh >> (8 * lane));
                const uint8_t* src = btype == 2 ? blk : in;
                for (uint32_t i = lane; i < body; i += 64) out[pos + 3 + i] = src[i];
                pos += 3 + body; nblocks = 1; done = len;
            }
        }
        uint32_t sum = 0;
        if (status == CZ_OK && cks) {
            sum = (uint32_t)cze_xxh64(in, len);
            if (pos + 4 > cap) status = CZ_E_OUTPUT_TOO_SMALL;
            else { if (lane < 4) out[pos + lane] = (uint8_t)(sum >> (8 * lane)); pos += 4; }
        }
        if (lane == 0) {
            res->status = status; res->blocks = nblocks; res->bytes_read = done; res->bytes_written = pos;
            res->checksum = sum; res->flags = flags;
        }
    }
}

__global__ void __launch_bounds__(CZE_THREADS, 3) cz_compress_records_kernel(cz_enc_args a) {
    cz_enc_dargs d; d.dicts = nullptr; d.dict_index = nullptr; d.ndicts = 0; d.pad = 0;
    czr_records<false>(a, d);
}
__global__ void __launch_bounds__(CZE_THREADS, 3) cz_compress_records_dict_kernel(cz_enc_args a, cz_enc_dargs d) {
    czr_records<true>(a, d);
}
