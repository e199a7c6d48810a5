/*
 * czstd_encfastsplit.hip — CZ_COMPRESS_FAST_SPLIT: the fast level with the groups of one buffer on many workgroups.
 *
 * The frame is byte for byte the CZ_COMPRESS_FAST frame of czstd_encfast.hip.  Nothing in that format is carried from group to
 * group: every 32 KiB sub-block stands alone (no match source in front of it, no Treeless literals, no Repeat_Mode, the first
 * sequence writes its offset) and the Raw-group rule looks at one 128 KiB group.  So a work unit is one GROUP, whichever frame it
 * belongs to, and the only thing a group needs from its predecessor is where its blocks go.
 *
 * cz_compress_fast_plan_kernel (one workgroup): the scan of cz_compress_plan_kernel with this level's units per frame — one per
 * group, at least one, plus one checksum unit for a frame of more than one group with CZ_COMPRESS_CHECKSUM, numbered BEFORE that
 * frame's groups — into unit_base[n + 1] (64-bit); clears the three words of per-frame state.
 *
 * cz_compress_groups_fast_kernel: a persistent grid of 256-thread workgroups that claim units in increasing order from one 64-bit
 * counter.  A group unit is the body of one iteration of the fast kernel's group loop: wave w runs czq_block on sub-block w into
 * its own slot, one workgroup barrier, all threads sum the four sizes and apply the Raw-group rule.  Then the placement of
 * czstd_encsplit.hip: lane 0 waits until the frame's chain state says that group g - 1 has been placed, takes the output position
 * and the block count from it, checks out_cap, publishes the state for group g + 1 BEFORE the copy, and all threads copy the header
 * (group 0) and the group's blocks from the waves' slots to their final place.  No staging area: the blocks sit in the slots until
 * the barrier in front of the next claim.  The caller's region is only written at final positions and only with whole groups that
 * fit out_cap, so nothing past bytes_written is touched.
 *
 * The chain state is two 64-bit words per frame (agent scope), both state << 62 | groups placed << 40 | payload:
 *     word P   payload = the output position behind those groups (32 bits: cz_compress_bound(0xFFF00000) < 2^32)
 *     word B   payload = the blocks written for them (18 bits; a Raw group is ONE block, so blocks do not count groups)
 * Every update is an atomicMax and every read an agent-scope load: the group count only grows along the chain, so an open word only
 * grows, and a closing state (2: a group or the header did not fit out_cap, 3: a wait ran into its bound) outranks every open word
 * and stays.  Group g polls until BOTH words carry the count g, or either is closed.  Only group g - 1 ever writes the count g, and
 * it writes it into each word together with that word's payload in one atomic, so each word validates itself: whichever order the
 * two updates become visible in, a word that shows the count g holds the payload for g.  No fence and no ordering between the two
 * stores is needed; the bytes of the blocks go to disjoint places and are never read by another workgroup.  The third word is the
 * checksum unit's ready << 32 | value.  Whoever closes a frame first (atomicMax on P returned an open word) writes its result
 * record: the first group that does not fit, or a group whose wait expired; otherwise the last group does.
 *
 * PROGRESS, as in czstd_encsplit.hip: a unit only ever waits for a unit with a LOWER number (group g for group g - 1 of its frame,
 * the last group for its frame's checksum unit), units are claimed in increasing order, and only by workgroups that are already
 * running.  So the lowest-numbered unfinished unit is held by a running workgroup and waits for nothing unfinished; by induction
 * every wait ends, whatever the grid and however few workgroups are resident.  The waits are bounded all the same (CZE_WAIT_POLLS
 * polls of s_sleep); at the bound the frame ends with CZ_E_WAIT_EXPIRED and its successors see the closed word.
 *
 * Included behind czstd_encfast.hip; czq_block and its callees are instantiated with USER = 3, copies of this kernel's own, so that
 * the kernels in front of this file compile as they did without it.
 */
#define CZG_STATE(w) ((uint32_t)((w) >> 62))
#define CZG_GROUPS(w) ((uint32_t)((w) >> 40) & 0xFFFFu)
#define CZG_LOW(w) ((w) & ((1ull << 40) - 1ull))
#define CZG_WORD(state, groups, low) (((unsigned long long)(state) << 62) | ((unsigned long long)(groups) << 40) | (unsigned long long)(low))
#define CZG_FSTATE_WORDS 3u          /* per frame: word P, word B, the checksum word */

struct CzgShared {
    unsigned long long unit;
    uint64_t pos;
    uint32_t frame, local, skip, act, before, first, sum, ready;
};
__shared__ CzgShared czg;

/* groups of a frame of `len` bytes (an empty input and one that is too long are one unit) */
__device__ static inline uint32_t czg_groups(uint64_t len) {
    if (len >= 0xFFF00000ull || len <= CZQ_GROUP) return 1u;
    return (uint32_t)((len + CZQ_GROUP - 1u) / CZQ_GROUP);
}
__device__ static inline uint32_t czg_units(uint64_t len, uint32_t flags) {
    const uint32_t g = czg_groups(len);
    return g + (g > 1u && (flags & CZ_COMPRESS_CHECKSUM) ? 1u : 0u);
}

__global__ void __launch_bounds__(CZE_THREADS) cz_compress_fast_plan_kernel(const uint64_t* in_len, uint32_t n, uint32_t flags,
                                                                             unsigned long long* unit_base, unsigned long long* fstate) {
    __shared__ uint32_t wsum[CZE_WAVES];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    unsigned long long base = 0;                                        /* at most 2^32 frames x (2^15 + 1) units */
    for (uint64_t tile = 0; tile < n; tile += CZE_THREADS) {
        const uint64_t i = tile + t;
        const uint32_t u = i < n ? czg_units(in_len[i], flags) : 0u;
        if (i < n) for (uint32_t k = 0; k < CZG_FSTATE_WORDS; k++) fstate[CZG_FSTATE_WORDS * i + k] = 0;
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

/* lane 0: polls the two chain words until both carry `need` groups or one is closed; 0 when the wait ran into its bound */
__device__ static inline int czg_wait_chain(unsigned long long* chain, uint32_t need, unsigned long long* p, unsigned long long* b) {
    for (uint32_t polls = 0;; polls++) {
        const unsigned long long x = CZ_LD_AGENT(chain), y = CZ_LD_AGENT(chain + 1);
        const uint32_t closed = CZG_STATE(x) >= CZE_CH_TOO_SMALL || CZG_STATE(y) >= CZE_CH_TOO_SMALL;
        if (closed || (CZG_GROUPS(x) >= need && CZG_GROUPS(y) >= need)) { *p = x; *b = y; return 1; }
        if (polls >= CZE_WAIT_POLLS) return 0;
        __builtin_amdgcn_s_sleep(64);
    }
}

__global__ void __launch_bounds__(CZE_THREADS, 3) cz_compress_groups_fast_kernel(cz_encsplit_args sa) {
    const cz_enc_args& a = sa.a;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const unsigned long long units = sa.unit_base[a.n];
    if (t == 0) czg.unit = atomicAdd(sa.counter, 1ull);
    __syncthreads();
    if (czg.unit >= units) return;                                      /* a workgroup without work */
    czq_predefined<3>();
    uint8_t* scr = a.scratch + (uint64_t)blockIdx.x * a.scratch_stride;
    uint8_t* slot = scr + wave * CZQ_SLOT_BYTES;
    CzqWave& S = czq.w[wave];
    for (uint32_t claimed = 1;; claimed = 0) {
        if (!claimed) { __syncthreads(); if (t == 0) czg.unit = atomicAdd(sa.counter, 1ull); }
        __syncthreads();
        const unsigned long long unit = czg.unit;
        if (unit >= units) break;
        /* the frame of the unit: the last f with unit_base[f] <= unit; a closed frame's later groups have nothing to do */
        if (t == 0) {
            uint32_t lo = 0, hi = a.n - 1;
            while (lo < hi) { const uint32_t mid = lo + (hi - lo + 1) / 2; if (sa.unit_base[mid] <= unit) lo = mid; else hi = mid - 1; }
            czg.frame = lo; czg.local = (uint32_t)(unit - sa.unit_base[lo]);
            czg.skip = CZG_STATE(CZ_LD_AGENT(&sa.fstate[CZG_FSTATE_WORDS * (uint64_t)lo])) >= CZE_CH_TOO_SMALL;
        }
        __syncthreads();
        const uint32_t f = cz_uni(czg.frame), local = cz_uni(czg.local);   /* (uniform: what depends on them stays in scalar registers) */
        if (czg.skip) continue;
        const uint8_t* in = a.in_base + a.in_off[f];
        const uint64_t len64 = a.in_len[f];
        uint8_t* out = a.out_base + a.out_off[f];
        const uint64_t cap = a.out_cap[f];
        cz_compress_result* res = a.results + f;
        unsigned long long* chain = &sa.fstate[CZG_FSTATE_WORDS * (uint64_t)f];
        const uint32_t cks = a.flags & CZ_COMPRESS_CHECKSUM, flags = cks | CZ_COMPRESS_FAST_SPLIT;
        if (len64 >= 0xFFF00000ull) {                                   /* positions are 32-bit */
            if (t == 0) { res->status = CZ_E_INVALID_ARG; res->blocks = 0; res->bytes_read = 0; res->bytes_written = 0; res->checksum = 0; res->flags = flags; }
            continue;
        }
        const uint32_t len = (uint32_t)len64, multi = len > CZQ_GROUP;
        if (multi && cks && local == 0) {                               /* the checksum unit: one wave, off the chain's path */
            if (wave == 0) { const uint64_t x = cze_xxh64(in, len); if (t == 0) CZ_ST_AGENT(chain + 2, (1ull << 32) | (uint32_t)x); }
            continue;
        }
        const uint32_t g = local - (multi && cks ? 1u : 0u);
        const uint32_t g0 = g * CZQ_GROUP, g1 = len - g0 < CZQ_GROUP ? len : g0 + CZQ_GROUP, gsize = g1 - g0;
        const uint32_t last_group = g1 == len;
        /* the group's blocks, each in its wave's slot; an empty input is one empty last Raw block */
        uint32_t total = 3, nb = 1, raw_group = 0;
        if (len) {
            const uint32_t s0 = g0 + wave * CZQ_SUB;
            uint32_t mine = CZQ_NONE;
            if (s0 < g1) mine = czq_block<3>(S, in, s0, g1 - s0 < CZQ_SUB ? g1 : s0 + CZQ_SUB, slot, slot + CZQ_SCR_BLK);
            if (lane == 0) czq.bres[0][wave] = mine;
            __syncthreads();                                            /* the group's one barrier */
            total = 0; nb = 0;
            for (uint32_t w = 0; w < CZE_WAVES; w++) { const uint32_t r = czq.bres[0][w]; if (r != CZQ_NONE) { total += 3u + (r & 0xFFFFFFu); nb++; } }
            raw_group = total > 3u + gsize;
            if (raw_group) { total = 3u + gsize; nb = 1; }
        }
        /* frame header (group 0) */
        uint8_t hdr[14]; uint32_t hl = 0;
        if (g == 0) {
            const uint32_t single = len <= (1u << 20);
            hdr[hl++] = 0x28; hdr[hl++] = 0xB5; hdr[hl++] = 0x2F; hdr[hl++] = 0xFD;
            const uint32_t fcs_flag = single && len < 256 ? 0u : (len >= 256 && len < 65536 + 256 ? 1u : 2u);
            hdr[hl++] = (uint8_t)((fcs_flag << 6) | (single << 5) | (cks ? 4u : 0u));
            if (!single) hdr[hl++] = (uint8_t)((20 - 10) << 3);        /* Window_Descriptor: 1 MiB */
            if (fcs_flag == 0) hdr[hl++] = (uint8_t)len;
            else if (fcs_flag == 1) { hdr[hl++] = (uint8_t)(len - 256); hdr[hl++] = (uint8_t)((len - 256) >> 8); }
            else for (int i = 0; i < 4; i++) hdr[hl++] = (uint8_t)(len >> (8 * i));
        }
        /* lane 0: where the group goes (act 0: nowhere, the frame is closed; 1: placed; else the state that closes the frame here)
           and the words for the successor — published before the copy */
        if (t == 0) {
            unsigned long long p = 0, b = 0; uint64_t pos = 0; uint32_t act = 1, before = 0;
            if (g == 0) { if (hl <= cap) pos = hl; else act = (uint32_t)CZE_CH_TOO_SMALL; }
            else if (!czg_wait_chain(chain, g, &p, &b)) act = (uint32_t)CZE_CH_EXPIRED;
            else if (CZG_STATE(p) >= CZE_CH_TOO_SMALL || CZG_STATE(b) >= CZE_CH_TOO_SMALL) act = 0;
            else { pos = CZG_LOW(p); before = (uint32_t)CZG_LOW(b); }
            if (act == 1) {
                if (pos + total > cap) act = (uint32_t)CZE_CH_TOO_SMALL;
                else if (!last_group) {
                    (void)atomicMax(chain, CZG_WORD(0, g + 1u, pos + total));
                    (void)atomicMax(chain + 1, CZG_WORD(0, g + 1u, before + nb));
                }
            }
            uint32_t first = 0;
            if (act >= CZE_CH_TOO_SMALL) {
                first = CZG_STATE(atomicMax(chain, CZG_WORD(act, g, pos))) < CZE_CH_TOO_SMALL;
                (void)atomicMax(chain + 1, CZG_WORD(act, g, before));
            }
            czg.pos = pos; czg.act = act; czg.before = before; czg.first = first;
        }
        __syncthreads();
        const uint32_t act = cz_uni(czg.act), before = cz_uni(czg.before);
        uint64_t pos = czg.pos;
        if (act == 0) continue;
        if (act == CZE_CH_EXPIRED) {                                    /* where the predecessors stand is not known */
            if (t == 0 && czg.first) { res->status = CZ_E_WAIT_EXPIRED; res->blocks = 0; res->bytes_read = 0; res->bytes_written = 0; res->checksum = 0; res->flags = flags; }
            continue;
        }
        if (g == 0 && hl <= cap) for (uint32_t i = t; i < hl; i += CZE_THREADS) out[i] = hdr[i];
        if (act == CZE_CH_TOO_SMALL) {                                  /* the frame ends in front of this group */
            if (t == 0 && czg.first) {
                res->status = CZ_E_OUTPUT_TOO_SMALL; res->blocks = before; res->bytes_read = g0; res->bytes_written = pos;
                res->checksum = 0; res->flags = flags;
            }
            continue;
        }
        if (!len) { if (t < 3) out[pos + t] = t == 0 ? 1 : 0; }
        else if (raw_group) {
            const uint32_t bh = last_group | (gsize << 3);
            if (t < 3) out[pos + t] = (uint8_t)(bh >> (8 * t));
            cze_copy(out + pos + 3, in + g0, gsize);
        } else {
            uint64_t o = pos;
            for (uint32_t w = 0; w < nb; w++) {
                const uint32_t r = czq.bres[0][w], btype = r >> 24, body = r & 0xFFFFFFu;
                const uint32_t b0 = g0 + w * CZQ_SUB, bsize = g1 - b0 < CZQ_SUB ? g1 - b0 : CZQ_SUB;
                const uint32_t bh = (last_group && w + 1 == nb ? 1u : 0u) | (btype << 1) | ((btype == 2 ? body : bsize) << 3);
                if (t < 3) out[o + t] = (uint8_t)(bh >> (8 * t));
                cze_copy(out + o + 3, btype == 2 ? scr + w * CZQ_SLOT_BYTES + CZQ_SCR_BLK : in + b0, body);
                o += 3u + body;
            }
        }
        pos += total;
        if (!last_group) continue;
        /* the last group: the checksum (a frame of several groups gets it from its checksum unit), then the result record */
        int status = CZ_OK; uint32_t sum = 0;
        if (cks) {
            if (!multi) { if (wave == 0) { const uint64_t x = cze_xxh64(in, len); if (t == 0) { czg.sum = (uint32_t)x; czg.ready = 1; } } }
            else if (t == 0) {
                /* XXH64 is serial over the input: the bound grows with it (64 bytes per poll) */
                const uint32_t bound = CZE_WAIT_POLLS + (len >> 6);
                unsigned long long w = 0;
                for (uint32_t polls = 0;; polls++) {
                    w = CZ_LD_AGENT(chain + 2);
                    if (w >> 32) break;
                    if (polls >= bound) break;
                    __builtin_amdgcn_s_sleep(64);
                }
                czg.sum = (uint32_t)w;
                czg.ready = (uint32_t)(w >> 32);                        /* 0: the wait ran into its bound */
            }
            __syncthreads();
            sum = czg.sum;
            if (!czg.ready) {
                if (t == 0) {
                    (void)atomicMax(chain, CZG_WORD(CZE_CH_EXPIRED, 0, 0));
                    (void)atomicMax(chain + 1, CZG_WORD(CZE_CH_EXPIRED, 0, 0));
                    res->status = CZ_E_WAIT_EXPIRED; res->blocks = 0; res->bytes_read = 0; res->bytes_written = 0; res->checksum = 0; res->flags = flags;
                }
                continue;
            }
            if (pos + 4 > cap) status = CZ_E_OUTPUT_TOO_SMALL;
            else { if (t < 4) out[pos + t] = (uint8_t)(sum >> (8 * t)); pos += 4; }
        }
        if (t == 0) {
            res->status = status; res->blocks = before + nb; res->bytes_read = len; res->bytes_written = pos;
            res->checksum = sum; res->flags = flags;
        }
    }
}
