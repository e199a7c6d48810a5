/*
 * czstd_encsplit.hip — CZ_COMPRESS_SPLIT: one large buffer compressed by many workgroups into ONE standard frame.
 *
 * An input longer than one segment (CZE_SEG = CZE_SEG_BLOCKS blocks of 128 KiB) is cut into segments that different workgroups
 * compress at the same time.  The frame is what cz_compress_frames_kernel writes — the same header, blocks of at most 128 KiB each
 * Raw, RLE or Compressed, Last_Block on the final block, the optional checksum — except for the state a frame carries from block
 * to block, which a segment k > 0 cannot inherit from a neighbour that is still running:
 *     hash table      starts empty; then the CZE_OVERLAP input bytes in front of the segment are inserted (same hash, same atomicMax,
 *                     no verifying, no parsing).  Positions stay absolute, so matches reach back into earlier segments;
 *                     CZE_SEG + CZE_OVERLAP <= 1 MiB keeps every offset inside the window.
 *     offset history  starts as (0, 0, 0), which equals no offset: the segment's first sequence is written as offset + 3, and from
 *                     then on the top entry is known.  The encoder uses no other entry (Offset_Value 1 with literals only).
 * Segment 0 starts as a frame does (empty table, history 1, 4, 8), so it comes out byte for byte as the first CZE_SEG bytes of the
 * unsplit frame.  An input of at most one segment is ONE segment: its frame is the unsplit frame.  The bytes depend on the input and
 * the flags alone, never on the batch, the grid or timing.
 *
 * cz_compress_plan_kernel (one workgroup): units per frame — one per segment, plus one checksum unit for a split frame with
 * CZ_COMPRESS_CHECKSUM, numbered BEFORE that frame's segments — scanned into unit_base[n + 1] (64-bit); clears the per-frame state.
 *
 * cz_compress_segments_kernel: a persistent grid of 256-thread workgroups that claim units in increasing order from one 64-bit
 * counter; a workgroup that finds none exits.  A segment unit runs the per-block pipeline of czstd_enc.hip over its blocks into a
 * staging buffer in the workgroup's own scratch (headers and bodies), then waits for the frame's chain word to say that segment
 * k - 1 has been placed, takes the output position from it, publishes its own end position, and copies its blocks to their final
 * place with all threads.  The caller's region is only ever written at final positions, and only with whole blocks that fit out_cap,
 * so nothing past bytes_written is touched.
 *
 * The chain word (64 bits per frame, agent scope): state << 61 | blocks placed << 40 | output position.  Every update is an
 * atomicMax: positions and block counts only grow along the chain, and a closing state (2: a block did not fit out_cap, 3: a wait
 * ran into its bound) outranks every open word and stays.  The word is all a successor reads of its predecessor — the bytes go
 * to disjoint places — so the polls are relaxed agent-scope loads and no fence is needed; a segment publishes BEFORE it copies, so
 * the chain costs a successor one poll, not a copy.  Whoever closes a frame first (atomicMax returned an open word) writes its result
 * record; otherwise the last segment does.
 *
 * PROGRESS.  A unit only ever waits for a unit with a LOWER number: segment k for segment k - 1 of its frame, the last segment for
 * its frame's checksum unit.  Units are claimed in increasing order, and only by workgroups that are already running.  So the
 * lowest-numbered unfinished unit is always held by a running workgroup and waits for nothing unfinished: it finishes, and by
 * induction every wait ends, whatever the grid and however few workgroups are resident.  The waits are bounded all the same
 * (CZE_WAIT_POLLS polls of s_sleep, seconds); at the bound the frame ends with CZ_E_WAIT_EXPIRED and its successors see the closed word.
 *
 * The kernel has its own per-block function (cze_seg_block) next to the bodies of czstd_enc.hip; those two kernels are untouched.
 * Included behind czstd_enc.hip.  CZE_SEG_BLOCKS and CZE_OVERLAP can be set with -D (the emulator builds one-block segments).
 */
/* S = 512 KiB and W = 512 KiB: the fastest of the twelve pairs measured, and within the size rule */
#ifndef CZE_SEG_BLOCKS
#define CZE_SEG_BLOCKS 4u
#endif
#ifndef CZE_OVERLAP
#define CZE_OVERLAP (512u * 1024u)
#endif
#define CZE_SEG (CZE_SEG_BLOCKS * CZE_BLOCK)
static_assert(CZE_SEG_BLOCKS >= 1u && CZE_SEG_BLOCKS <= 8u, "a segment is 1 to 8 blocks");
static_assert((uint64_t)CZE_SEG + CZE_OVERLAP <= CZE_WINDOW, "S + W must stay inside the 1 MiB window");
/* the workgroup's scratch: that of cz_compress_frames_kernel, then the staged segment (S + 3 bytes per block; a block under
   construction may run 3 bytes past its input size before it falls back to Raw) */
#define CZE_SCR_STAGE CZE_SCRATCH_BYTES
#define CZE_SPLIT_SCRATCH_BYTES (CZE_SCRATCH_BYTES + CZE_SEG + 64u + 4096u)
#define CZE_WAIT_POLLS (1u << 21)           /* x >= 4 096 clocks of s_sleep: >= 3 s */

#define CZE_CH_TOO_SMALL 2ull
#define CZE_CH_EXPIRED 3ull
#define CZE_CH_STATE(w) ((uint32_t)((w) >> 61))
#define CZE_CH_BLOCKS(w) ((uint32_t)((w) >> 40) & 0x1FFFFFu)
#define CZE_CH_POS(w) ((w) & ((1ull << 40) - 1ull))
#define CZE_CH_WORD(state, blocks, pos) (((unsigned long long)(state) << 61) | ((unsigned long long)(blocks) << 40) | (unsigned long long)(pos))

struct cz_encsplit_args {
    cz_enc_args a;                      /* work_counter is not used: units come from `counter` */
    unsigned long long* unit_base;      /* n + 1 */
    unsigned long long* fstate;         /* per frame: the chain word, then ready << 32 | the checksum */
    unsigned long long* counter;
};

struct CzeSplitShared {
    unsigned long long unit, word;
    uint32_t frame, local, skip, act, nfit, first, sum;
    uint32_t bsz[CZE_SEG_BLOCKS];
};
__shared__ CzeSplitShared czs;

/* work units of a frame of `len` bytes */
__device__ static inline uint32_t cze_split_units(uint64_t len, uint32_t flags) {
    if (len >= 0xFFF00000ull || len <= CZE_SEG) return 1u;             /* (an input that long fails in its one unit) */
    return (uint32_t)((len + CZE_SEG - 1u) / CZE_SEG) + ((flags & CZ_COMPRESS_CHECKSUM) ? 1u : 0u);
}

__global__ void __launch_bounds__(CZE_THREADS) cz_compress_plan_kernel(const uint64_t* in_len, uint32_t n, uint32_t flags,
                                                                        unsigned long long* unit_base, unsigned long long* fstate) {
    __shared__ uint32_t wsum[CZE_WAVES];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    unsigned long long base = 0;                                        /* at most 2^32 frames x 2^15 units */
    for (uint64_t tile = 0; tile < n; tile += CZE_THREADS) {
        const uint64_t i = tile + t;
        const uint32_t u = i < n ? cze_split_units(in_len[i], flags) : 0u;
        if (i < n) { fstate[2 * i] = 0; fstate[2 * i + 1] = 0; }
        uint32_t x = u;                                                 /* a tile's sum stays below 2^24 */
        for (unsigned d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d); if (lane >= d) x += y; }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < CZE_WAVES; w++) { const uint32_t s = wsum[w]; if (w < wave) before += s; all += s; }
        __syncthreads();
        if (i < n) unit_base[i] = base + before + x - u;
        base += all;
    }
    if (t == 0) unit_base[n] = base;
}

/* all threads: n bytes, any alignment, 4 at a time */
__device__ static inline void cze_copy(uint8_t* dst, const uint8_t* src, uint32_t n) {
    const uint32_t t = threadIdx.x, n4 = n & ~3u;
    for (uint32_t i = 4u * t; i < n4; i += 4u * CZE_THREADS) { uint32_t v; __builtin_memcpy(&v, src + i, 4); __builtin_memcpy(dst + i, &v, 4); }
    if (t < n - n4) dst[n4 + t] = src[n4 + t];
}

/* One block [b0, b1) of the input into st: the 3-byte header, then the body, Raw, RLE or Compressed, whichever is smallest.  The
   pipeline of cz_compress_frames_kernel, step for step, on the workgroup's table (cze.htab) and offset history (cze.rep), which a
   block that is not written Compressed leaves as it found it.  Returns 3 + the body's length (every thread). */
__device__ static uint32_t cze_seg_block(const uint8_t* in, uint32_t b0, uint32_t b1, uint32_t last, uint8_t* st, uint8_t* lit, CzeSeq* seqs,
                                         uint32_t* hufw) {
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
        const uint32_t lsz = cze_literals<false, 1>(lit, nlit, blk, hufw, nullptr, 0u, nullptr);
        if (lsz < bsize) {
            if (t == 0) cze.csize = lsz + cze_sequences<false, 1>(seqs, nseq, nsl, blk + lsz, bsize - lsz, nullptr, 0u, nullptr);
            __syncthreads();
            csize = cze.csize;
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

/* lane 0: polls *p until the frame is closed or `need` blocks have been placed; 0 when the wait ran into its bound */
__device__ static inline int cze_wait_chain(unsigned long long* p, uint32_t need, unsigned long long* out) {
    for (uint32_t polls = 0;; polls++) {
        const unsigned long long w = CZ_LD_AGENT(p);
        if (CZE_CH_STATE(w) >= CZE_CH_TOO_SMALL || CZE_CH_BLOCKS(w) >= need) { *out = w; return 1; }
        if (polls >= CZE_WAIT_POLLS) return 0;
        __builtin_amdgcn_s_sleep(64);
    }
}

__global__ void __launch_bounds__(CZE_THREADS) cz_compress_segments_kernel(cz_encsplit_args sa) {
    const cz_enc_args& a = sa.a;
    const uint32_t t = threadIdx.x, wave = t >> 6;
    const unsigned long long total = sa.unit_base[a.n];
    if (t == 0) czs.unit = atomicAdd(sa.counter, 1ull);
    __syncthreads();
    if (czs.unit >= total) return;                                      /* a workgroup without work */
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
    uint8_t* stage = scr + CZE_SCR_STAGE;
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
            if (t == 0) { res->status = CZ_E_INVALID_ARG; res->blocks = 0; res->bytes_read = 0; res->bytes_written = 0; res->checksum = 0; res->flags = cks; }
            continue;
        }
        const uint32_t len = (uint32_t)len64, split = len > CZE_SEG;
        const uint32_t flags = cks | (split ? CZ_COMPRESS_SPLIT : 0u);
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
            const uint32_t sz = cze_seg_block(in, b0, b1, b1 == len, stage + staged, lit, seqs, hufw);
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
