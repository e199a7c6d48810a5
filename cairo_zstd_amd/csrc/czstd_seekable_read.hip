/*
 * czstd_seekable_read.hip — byte ranges out of a seekable stream on the device: cz_seekable_index_create_device,
 * cz_seekable_locate_device and cz_seekable_gather_device.  "Content" is the frames' decompressed bytes in frame order; a range is
 * (offset, length) in content coordinates.
 *
 * INDEX, once per stream: cz_seekable_open_kernel validates the table (an open of no frames: the validation is that kernel's, not a
 * copy of it), then cz_seekable_index_kernel (one workgroup) scans both size columns of the unaligned table in 64 bits into
 * comp[0 .. n] and cont[0 .. n], copies the checksums and zeroes the per-frame scratch reach[0 .. n).  The table is not read again.
 *
 * LOCATE is two launches and a synchronise (the host needs k for the decode launch).
 *
 * cz_seekable_locate_kernel: one thread per range, any number of workgroups.  A range outside the content records its index in
 * *bad (atomicMax of 2^32 - 1 - j: the lowest index wins).  Any other non-empty range finds the frames fa and fb of its first and
 * last byte — the last frame that starts at or in front of the byte, which is never an empty one — and records
 * atomicMax(&reach[fa], fb + 1), and (fa, fb + 1) in rng[] for the spans.  Frame i is then covered exactly when the running maximum
 * of reach[0 .. i] exceeds i.
 *
 * cz_seekable_select_kernel (one workgroup): a prefix maximum over reach, a compaction scan of the covered frames that are not empty
 * and a scan of their sizes rounded up to out_align; reach[i] becomes the frame's rank + 1 and sel_off[rank] its out_off.  Then the
 * ranges: the scan of their lengths (dst_off) and, from rng[], reach[] and sel_off[], the spans.  Last, one pass that writes the
 * per-frame arrays from the ranks and zeroes reach[] again.  A bad range or k > frames_cap writes no array; reach[] and *bad are
 * clean again on every path.
 *
 * cz_seekable_ranges_kernel (GATHER, the hot path) is built like cz_seekable_gather_kernel: the DESTINATION, the ranges back to
 * back, is cut into tiles of 16-byte vectors aligned in memory, a persistent grid takes tiles blockIdx.x, + gridDim.x, ...  Per tile
 * two waves find the ranges of its first and last byte by binary search over spans[].dst_off; every thread then finds its vector's
 * range between the two (the LAST range that starts at or in front of the byte: empty ranges share a dst_off with their successor
 * and are never it) and, within the span's selected frames, the frame that holds the byte.  A vector inside one range and one frame
 * is ONE 16-byte load at the source's own alignment and one aligned 16-byte store; a vector that crosses a range or a frame or hangs
 * over an end of the destination is put together and stored byte by byte.  No load leaves the bytes of a selected frame that a range
 * asks for, no store leaves [0, dst_bytes).
 *
 * Included behind czstd_seekable.hip, whose helpers (czs_scan, czs_find, czs_ld32) it uses, with its own statics only.
 */
#define CZR_BAD_NONE 0u
#define CZR_ROWS 8u                          /* rows of CZS_THREADS frames per turn of the selection's last pass */

struct cz_seekable_index_args {
    const uint8_t* stream; uint64_t stream_len, n; uint32_t E;
    unsigned long long* comp; unsigned long long* cont; uint32_t* sums; uint32_t* reach;
};
/* the table was validated by cz_seekable_open_kernel: n entries of E bytes end 9 bytes in front of the stream's end */
__global__ void __launch_bounds__(CZS_THREADS) cz_seekable_index_kernel(cz_seekable_index_args a) {
    const uint32_t t = threadIdx.x, E = a.E; const uint64_t n = a.n;
    const uint8_t* ent = a.stream + (a.stream_len - (17 + n * E)) + 8;
    uint64_t cbase = 0, dbase = 0;
    for (uint64_t tile = 0; tile < n; tile += CZS_THREADS * CZS_ITEMS) {
        const uint64_t i0 = tile + (uint64_t)t * CZS_ITEMS;
        uint32_t c[CZS_ITEMS], d[CZS_ITEMS], x[CZS_ITEMS]; uint64_t csum = 0, dsum = 0;
        for (uint32_t k = 0; k < CZS_ITEMS; k++) {                      /* (all loads in flight together) */
            const uint8_t* e = ent + (i0 + k < n ? i0 + k : n - 1) * E;
            c[k] = czs_ld32(e); d[k] = czs_ld32(e + 4); x[k] = E == 12 ? czs_ld32(e + 8) : 0u;
        }
        for (uint32_t k = 0; k < CZS_ITEMS; k++) {
            if (i0 + k >= n) { c[k] = 0; d[k] = 0; }
            csum += c[k]; dsum += d[k];
        }
        uint64_t call, dall;
        uint64_t ci = cbase + czs_scan(csum, &call), di = dbase + czs_scan(dsum, &dall);
        for (uint32_t k = 0; k < CZS_ITEMS; k++) {
            const uint64_t i = i0 + k;
            if (i < n) { a.comp[i] = ci; a.cont[i] = di; a.sums[i] = x[k]; a.reach[i] = 0; }
            ci += c[k]; di += d[k];
        }
        cbase += call; dbase += dall;
    }
    if (t == 0) { a.comp[n] = cbase; a.cont[n] = dbase; }
}

struct cz_seekable_locate_args {
    const unsigned long long* cont; uint64_t n; const uint64_t* range_off; const uint64_t* range_len; uint64_t m;
    uint32_t* reach; uint32_t* rng; uint32_t* bad;
};
__global__ void __launch_bounds__(CZS_THREADS) cz_seekable_locate_kernel(cz_seekable_locate_args a) {
    const uint64_t j = (uint64_t)blockIdx.x * CZS_THREADS + threadIdx.x;
    if (j >= a.m) return;
    const uint64_t content = a.cont[a.n], o = a.range_off[j], l = a.range_len[j];
    uint32_t fa = 0, fe = 0;                                            /* frames [fa, fe); fe = 0: the range is empty */
    if (o > content || l > content - o) atomicMax(a.bad, 0xFFFFFFFFu - (uint32_t)j);   /* (in this form o + l never wraps) */
    else if (l) {
        fa = czs_find(a.cont, 0, (uint32_t)a.n - 1, o);                 /* (l > 0 inside the content: n > 0) */
        fe = czs_find(a.cont, fa, (uint32_t)a.n - 1, o + (l - 1)) + 1;
        atomicMax(&a.reach[fa], fe);
    }
    a.rng[2 * j] = fa; a.rng[2 * j + 1] = fe;
}

/* exclusive prefix maximum of x over the workgroup's CZS_THREADS threads (0 in front of thread 0), *all = the maximum of all;
   every thread calls it */
__device__ static inline uint32_t czr_scan_max(uint32_t x, uint32_t* all) {
    __shared__ uint32_t wmax[CZS_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t s = x;
    for (unsigned d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(s, d); if (lane >= d && y > s) s = y; }
    uint32_t prev = __shfl_up(s, 1u);
    if (lane == 0) prev = 0;
    if (lane == 63) wmax[wave] = s;
    __syncthreads();
    uint32_t before = 0, top = 0;
    for (uint32_t w = 0; w < CZS_WAVES; w++) { const uint32_t v = wmax[w]; if (w < wave && v > before) before = v; if (v > top) top = v; }
    __syncthreads();
    *all = top;
    return before > prev ? before : prev;
}

struct cz_seekable_select_args {
    const unsigned long long* comp; const unsigned long long* cont; const uint32_t* sums; uint32_t* reach; unsigned long long* sel_off;
    const uint32_t* rng; uint32_t* bad; uint64_t n; uint32_t has_checksums, out_align; uint64_t frames_cap;
    const uint64_t* range_off; const uint64_t* range_len; uint64_t m;
    uint32_t* frame; uint64_t* in_off; uint64_t* in_len; uint64_t* out_off; uint64_t* out_cap; uint32_t* checksum; uint64_t* content_off;
    cz_seekable_span* spans; cz_seekable_read_info* info;
};
__global__ void __launch_bounds__(CZS_THREADS) cz_seekable_select_kernel(cz_seekable_select_args a) {
    __shared__ uint32_t head[1];
    const uint32_t t = threadIdx.x; const uint64_t n = a.n, align = a.out_align;
    if (t == 0) { head[0] = *a.bad; *a.bad = CZR_BAD_NONE; }            /* (clean for the next locate) */
    __syncthreads();
    const uint32_t bad = cz_uni(head[0]);
    cz_seekable_read_info out;
    out.status = CZ_OK; out.reason = 0; out.frames = n; out.content_bytes = a.cont[n]; out.selected = 0; out.out_bytes = 0; out.dst_bytes = 0;
    out.detail = 0; out.has_checksums = a.has_checksums; out.reserved = 0;
    if (bad != CZR_BAD_NONE) {                                          /* the ranges that were good have left their marks */
        for (uint64_t i = t; i < n; i += CZS_THREADS) a.reach[i] = 0;
        out.status = CZ_E_INVALID_ARG; out.detail = 0xFFFFFFFFu - bad;
        if (t == 0) *a.info = out;
        return;
    }
    /* the selection: reach[i] := rank + 1 of a covered frame that is not empty, else 0; sel_off[rank] := its out_off */
    uint32_t carry = 0; uint64_t ranks = 0, pos = 0, last_s = ~0ull, last_need = 0;
    for (uint64_t tile = 0; tile < n; tile += CZS_THREADS * CZS_ITEMS) {
        const uint64_t i0 = tile + (uint64_t)t * CZS_ITEMS;
        uint32_t r[CZS_ITEMS]; uint64_t c[CZS_ITEMS + 1];
        for (uint32_t k = 0; k < CZS_ITEMS; k++) r[k] = a.reach[i0 + k < n ? i0 + k : n - 1];   /* (all loads in flight together) */
        for (uint32_t k = 0; k <= CZS_ITEMS; k++) c[k] = a.cont[i0 + k < n ? i0 + k : n];
        uint32_t top = 0, all;
        for (uint32_t k = 0; k < CZS_ITEMS; k++) if (i0 + k < n && r[k] > top) top = r[k];
        uint32_t run = czr_scan_max(top, &all);
        if (carry > run) run = carry;
        uint32_t mask = 0; uint64_t cnt = 0, psum = 0;
        for (uint32_t k = 0; k < CZS_ITEMS; k++) {
            const uint64_t i = i0 + k, d = c[k + 1] - c[k];
            if (i < n && r[k] > run) run = r[k];
            if (i < n && run > i && d) { mask |= 1u << k; cnt++; psum += (d + align - 1) & ~(align - 1); }
        }
        uint64_t call, pall;
        uint64_t s = ranks + czs_scan(cnt, &call), po = pos + czs_scan(psum, &pall);
        for (uint32_t k = 0; k < CZS_ITEMS; k++) {
            const uint64_t i = i0 + k, d = c[k + 1] - c[k];
            if ((mask >> k) & 1u) {
                a.reach[i] = (uint32_t)s + 1; a.sel_off[s] = po;
                last_s = s; last_need = po + d;
                s++; po += (d + align - 1) & ~(align - 1);
            } else if (i < n) a.reach[i] = 0;
        }
        ranks += call; pos += pall;
        if (all > carry) carry = all;
    }
    const uint64_t k = ranks;
    uint64_t need;
    (void)czs_scan(last_s + 1 == k && k ? last_need : 0, &need);        /* (one thread holds it) */
    const bool per_frame = a.frame || a.in_off || a.in_len || a.out_off || a.out_cap || a.checksum || a.content_off;
    const bool small = per_frame && k > a.frames_cap;
    __syncthreads();                                                    /* reach[] and sel_off[] are read by other threads now */
    /* the ranges: dst_off is the scan of their lengths; the rest of a span comes from rng[], the ranks and sel_off[] */
    uint64_t dbase = 0;
    for (uint64_t tile = 0; tile < a.m; tile += CZS_THREADS * CZS_ITEMS) {
        const uint64_t j0 = tile + (uint64_t)t * CZS_ITEMS;
        uint64_t len[CZS_ITEMS], sum = 0, dall;
        for (uint32_t q = 0; q < CZS_ITEMS; q++) { len[q] = j0 + q < a.m ? a.range_len[j0 + q] : 0; sum += len[q]; }
        uint64_t at = dbase + czs_scan(sum, &dall);
        if (a.spans && !small)
            for (uint32_t q = 0; q < CZS_ITEMS; q++) {
                const uint64_t j = j0 + q;
                if (j >= a.m) continue;
                cz_seekable_span sp; sp.dst_off = at; sp.src_off = 0; sp.sel_first = 0; sp.sel_count = 0;
                const uint32_t fa = a.rng[2 * j], fe = a.rng[2 * j + 1];
                if (fe) {
                    const uint32_t ra = a.reach[fa], rb = a.reach[fe - 1];
                    sp.sel_first = ra - 1; sp.sel_count = rb - ra + 1;
                    sp.src_off = a.sel_off[ra - 1] + (a.range_off[j] - a.cont[fa]);
                }
                a.spans[j] = sp;
                at += len[q];
            }
        dbase += dall;
    }
    __syncthreads();                                                    /* reach[] is zeroed now */
    for (uint64_t base = 0; base < n; base += CZS_THREADS * CZR_ROWS) {  /* (rows of neighbouring lanes, all loads in flight together) */
        uint32_t r[CZR_ROWS];
        for (uint32_t q = 0; q < CZR_ROWS; q++) { const uint64_t i = base + q * CZS_THREADS + t; r[q] = i < n ? a.reach[i] : 0u; }
        for (uint32_t q = 0; q < CZR_ROWS; q++) {
            if (!r[q]) continue;
            const uint64_t i = base + q * CZS_THREADS + t, s = r[q] - 1;
            a.reach[i] = 0;
            if (!per_frame || small) continue;
            if (a.frame) a.frame[s] = (uint32_t)i;
            if (a.in_off) a.in_off[s] = a.comp[i];
            if (a.in_len) a.in_len[s] = a.comp[i + 1] - a.comp[i];
            if (a.out_off) a.out_off[s] = a.sel_off[s];
            if (a.out_cap) a.out_cap[s] = a.cont[i + 1] - a.cont[i];
            if (a.checksum) a.checksum[s] = a.sums[i];
            if (a.content_off) a.content_off[s] = a.cont[i];
        }
    }
    out.status = small ? CZ_E_OUTPUT_TOO_SMALL : CZ_OK; out.selected = k; out.out_bytes = need; out.dst_bytes = dbase;
    if (t == 0) *a.info = out;
}

struct cz_seekable_ranges_args {
    const uint8_t* decoded; const unsigned long long* out_off; const unsigned long long* content_off;
    const uint64_t* range_off; const uint64_t* range_len; const cz_seekable_span* spans; uint32_t m;
    uint8_t* dst; uint64_t dst_bytes;
};
/* the last j in [lo, hi] with spans[j].dst_off <= p (spans[lo].dst_off <= p) */
__device__ static inline uint32_t czr_find_span(const cz_seekable_span* spans, uint32_t lo, uint32_t hi, uint64_t p) {
    while (lo < hi) { const uint32_t mid = lo + (hi - lo + 1) / 2; if (spans[mid].dst_off <= p) lo = mid; else hi = mid - 1; }
    return lo;
}

__global__ void __launch_bounds__(CZS_THREADS) cz_seekable_ranges_kernel(cz_seekable_ranges_args a) {
    __shared__ uint32_t edge[2];
    const uint32_t t = threadIdx.x;
    const uint64_t total = a.dst_bytes;
    const uint32_t mis = (uint32_t)((uintptr_t)a.dst & 15u);
    uint8_t* const vec0 = a.dst - mis;                                  /* 16-byte aligned; vector v is vec0 + 16 v */
    const uint64_t vecs = (mis + total + 15) / 16, tiles = (vecs + CZS_TILE_VECS - 1) / CZS_TILE_VECS;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t v0 = tile * CZS_TILE_VECS, v1 = v0 + CZS_TILE_VECS < vecs ? v0 + CZS_TILE_VECS : vecs;
        /* destination positions of the tile: [p0, p1); the ranges of its first and last byte, found by two waves side by side */
        const uint64_t p0 = v0 * 16 > mis ? v0 * 16 - mis : 0, p1 = v1 * 16 - mis < total ? v1 * 16 - mis : total;
        if (t == 0 || t == 64) edge[t >> 6] = czr_find_span(a.spans, 0, a.m - 1, t == 0 ? p0 : p1 - 1);
        __syncthreads();
        const uint32_t jlo = edge[0], jhi = edge[1];
        for (uint64_t v = v0 + t; v < v1; v += CZS_THREADS) {
            const uint64_t b0 = v * 16, q0 = b0 > mis ? b0 - mis : 0, q1 = b0 + 16 - mis < total ? b0 + 16 - mis : total;   /* [q0, q1) */
            uint8_t* dst = vec0 + b0;
            uint32_t j = czr_find_span(a.spans, jlo, jhi, q0);          /* (not an empty one: see above) */
            uint64_t rs = a.spans[j].dst_off, re = rs + a.range_len[j], ro = a.range_off[j];
            uint32_t s = a.spans[j].sel_first, se = s + a.spans[j].sel_count;
            /* the piece: the selected frame of the span that holds content byte c; it ends where the next selected frame starts
               (only empty frames lie between two of a span) or, for the span's last frame, not in front of the range's end */
            uint64_t c = ro + (q0 - rs);
            s = czs_find(a.content_off, s, se - 1, c);
            uint64_t cs = a.content_off[s], ce = s + 1 < se ? a.content_off[s + 1] : ~0ull;
            if (q1 - q0 == 16 && q1 <= re && c + 16 <= ce) {            /* a whole vector inside one range and one frame */
                uint4 x; memcpy(&x, a.decoded + a.out_off[s] + (c - cs), 16);
                *(uint4*)dst = x;
                continue;
            }
            for (uint64_t q = q0; q < q1; q++) {                        /* byte by byte, as in cz_seekable_gather_kernel */
                while (q >= re) {                                       /* the next range that is not empty */
                    j++; rs = re; re = rs + a.range_len[j];
                    if (re == rs) continue;
                    ro = a.range_off[j]; s = a.spans[j].sel_first; se = s + a.spans[j].sel_count;
                    cs = a.content_off[s]; ce = s + 1 < se ? a.content_off[s + 1] : ~0ull;
                }
                c = ro + (q - rs);
                while (c >= ce) { s++; cs = ce; ce = s + 1 < se ? a.content_off[s + 1] : ~0ull; }
                dst[q + mis - b0] = a.decoded[a.out_off[s] + (c - cs)];
            }
        }
        __syncthreads();                                                /* edge[] is written again */
    }
}
