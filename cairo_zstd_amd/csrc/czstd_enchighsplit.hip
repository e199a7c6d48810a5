/*
 * czstd_enchighsplit.hip — CZ_COMPRESS_HIGH_SPLIT: the high-ratio level with the segments of one buffer on many workgroups
 * (DESIGN.md §10.9).
 *
 * cz_compress_segments_fse_kernel (czstd_encfse.hip) around czh_block (czstd_enchigh.hip): the same units from the same plan
 * (cz_compress_plan_kernel), the same chain word, waits, staging buffer and publish-before-copy; czstd_encsplit.hip has the argument
 * for progress.  What a segment k > 0 cannot inherit from a neighbour that is still running it rebuilds or does without:
 *     match tables    BOTH start empty for every unit a workgroup claims, so a persistent workgroup never sees the entries of its
 *                     previous unit (cze_match would verify a stale hit against this input and take it: the bytes would depend on
 *                     which unit the workgroup had before).  Then the CZE_OVERLAP input bytes in front of the segment are inserted,
 *                     cze.htab for positions with 4 bytes left in the input and czh.htab8 for positions with 8, with the hashes and
 *                     the atomicMax of czh_block; no verifying, no parsing.
 *     offset history  starts as (0, 0, 0).  A 0 entry is never a candidate (czh_rep skips it, and 0 - 1 wraps above every
 *                     position) and equals no offset in the Offset_Value chain, so the segment's first sequence is explicit.  Every
 *                     update of the format is a push or a permutation of a prefix of the history, so the non-zero entries are
 *                     always a prefix of the decoder's real history, and all six repeat cases are used as entries become known.
 * Segment 0 starts as a frame does, so it comes out byte for byte as the first CZE_SEG bytes' worth of the CZ_COMPRESS_HIGH frame; an
 * input of at most one segment is ONE segment and its frame is that level's.  The result flags carry CZ_COMPRESS_HIGH_SPLIT whatever
 * the length.
 *
 * Included behind czstd_enchigh.hip.  czh_block, cze_match, cze_literals, czf_predefined and czf_sequences are instantiated with a
 * USER no other kernel has (5, 5, 5, 2, 2), so the kernels in front of this file compile as they did without it.
 */
__global__ void __launch_bounds__(CZE_THREADS) cz_compress_segments_high_kernel(cz_encsplit_args sa) {
    const cz_enc_args& a = sa.a;
    const uint32_t t = threadIdx.x, wave = t >> 6;
    const unsigned long long total = sa.unit_base[a.n];
    if (t == 0) czs.unit = atomicAdd(sa.counter, 1ull);
    __syncthreads();
    if (czs.unit >= total) return;                                      /* a workgroup without work */
    czf_predefined<2>();
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
        const uint32_t cks = a.flags & CZ_COMPRESS_CHECKSUM, flags = cks | CZ_COMPRESS_HIGH_SPLIT;
        if (len64 >= 0xFFF00000ull) {                                   /* positions are 32-bit */
            if (t == 0) { res->status = CZ_E_INVALID_ARG; res->blocks = 0; res->bytes_read = 0; res->bytes_written = 0; res->checksum = 0; res->flags = flags; }
            continue;
        }
        const uint32_t len = (uint32_t)len64, split = len > CZE_SEG;
        if (split && cks && local == 0) {                               /* the checksum unit: one wave, off the chain's path */
            if (wave == 0) { const uint64_t x = cze_xxh64(in, len); if (t == 0) CZ_ST_AGENT(chain + 1, (1ull << 32) | (uint32_t)x); }
            continue;
        }
        const uint32_t seg = local - (split && cks ? 1u : 0u);
        const uint32_t s0 = seg * CZE_SEG, s1 = len - s0 < CZE_SEG ? len : s0 + CZE_SEG;
        const uint32_t nb = len == 0 ? 1u : (s1 - s0 + CZE_BLOCK - 1) / CZE_BLOCK, blocks_before = seg * CZE_SEG_BLOCKS;
        const uint32_t last_seg = s1 == len;
        /* both tables: empty for every unit, then for a later segment the overlap in front of it */
        for (uint32_t k = t; k < (1u << CZE_HASH_LOG); k += CZE_THREADS) cze.htab[k] = 0;
        for (uint32_t k = t; k < (1u << CZH_HASH8_LOG); k += CZE_THREADS) czh.htab8[k] = 0;
        if (t == 0) { cze.rep[0] = seg ? 0u : 1u; cze.rep[1] = seg ? 0u : 4u; cze.rep[2] = seg ? 0u : 8u; }
        __syncthreads();
        if (seg) {
            for (uint32_t p = (s0 > CZE_OVERLAP ? s0 - CZE_OVERLAP : 0u) + t; p < s0; p += CZE_THREADS) {
                if (p + 4 <= len) atomicMax(&cze.htab[cze_hash(cze_ld4(in + p))], p + 1);
                if (p + 8 <= len) atomicMax(&czh.htab8[czh_hash8(in + p)], p + 1);
            }
            __syncthreads();
        }
        /* the blocks, staged */
        uint32_t staged = 0;
        for (uint32_t j = 0; j < nb; j++) {
            const uint32_t b0 = s0 + j * CZE_BLOCK, b1 = s1 - b0 < CZE_BLOCK ? s1 : b0 + CZE_BLOCK;
            const uint32_t sz = czh_block<5, 2>(in, b0, b1, b1 == len, stage + staged, lit, seqs, hufw, fscr);
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
