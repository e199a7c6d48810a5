/*
 * czstd_seekable.hip — seekable streams on the device: cz_seekable_pack_device and cz_seekable_open_device.
 *
 *     frame 0 | ... | frame n-1 | 0x184D2A5E | Frame_Size = n * E + 9 | n x { Compressed_Size, Decompressed_Size, [Checksum] } |
 *     Number_Of_Frames | Seek_Table_Descriptor (1 byte) | 0x8F92EAB1          — 32-bit little-endian fields, nothing aligned
 *
 * PACK is two launches on one stream; ordering comes from the stream alone and no workgroup waits for another.
 *
 * cz_seekable_plan_kernel (one workgroup): reads the n result records, decides what depends on them (a failed record, a size of 2^32
 * or more, a missing checksum; the need against stream_cap), scans bytes_written in 64 bits into plan[0 .. n] (plan[n] = the table's
 * offset), writes *info and the go word plan[n + 1].  It reads the records only, never a frame or the stream.
 *
 * cz_seekable_gather_kernel (the hot path): the DESTINATION is one contiguous range, and it, not the frames, is cut into equal
 * tiles, so 100 000 frames of 90 bytes and 64 frames of 1 MiB give every workgroup the same work.  The stream is seen as 16-byte
 * vectors aligned in memory (vector 0 holds the stream's first byte, wherever d_stream points); a tile is CZS_TILE_VECS of them, and a
 * persistent grid takes tiles blockIdx.x, + gridDim.x, ...  Per tile two waves find the frames of its first and last byte by binary
 * search over the scanned offsets; every thread then finds its vector's frame between the two.  A vector that lies inside one frame
 * is ONE 16-byte load at the source's own alignment (gfx950 takes unaligned global loads) and one aligned 16-byte store.  A vector
 * that crosses a frame boundary, reaches into the table or hangs over an end of the stream is put together and stored byte by byte,
 * the table's bytes from the records.  No load leaves a frame's [0, bytes_written), no store leaves [0, stream_bytes).
 *
 * OPEN is one launch: cz_seekable_open_kernel (one workgroup) reads the footer, validates in the order of the six reasons, sums both
 * size columns of the unaligned table in 64 bits (and the compressed sizes in front of `first`), and only when the sums agree with the
 * table's offset scans the range a tile at a time into the four arrays of cz_decode_batch_device.
 *
 * Included behind czstd_kernels.hip (cz_uni) with its own statics only: the kernels in front of this file compile as they did
 * without it.
 */
#define CZS_THREADS 256u
#define CZS_WAVES 4u
#define CZS_ITEMS 16u                       /* records or table entries per thread and tile in the scans */
#define CZS_TILE_VECS (2u * CZS_THREADS)     /* 16-byte vectors per tile: 8 KiB of the stream */
#define CZS_SKIP_MAGIC_D 0x184D2A5Eu
#define CZS_SEEK_MAGIC_D 0x8F92EAB1u
#define CZS_MAX_FRAMES 0x8000000u

__device__ static inline uint64_t czs_shfl_up64(uint64_t x, unsigned d) {
    const uint32_t lo = __shfl_up((uint32_t)x, d), hi = __shfl_up((uint32_t)(x >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}
/* exclusive prefix of x over the workgroup's CZS_THREADS threads, *all = their sum; every thread calls it */
__device__ static inline uint64_t czs_scan(uint64_t x, uint64_t* all) {
    __shared__ uint64_t wsum[CZS_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t s = x;
    for (unsigned d = 1; d < 64; d <<= 1) { const uint64_t y = czs_shfl_up64(s, d); if (lane >= d) s += y; }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    uint64_t before = 0, sum = 0;
    for (uint32_t w = 0; w < CZS_WAVES; w++) { const uint64_t v = wsum[w]; if (w < wave) before += v; sum += v; }
    __syncthreads();
    *all = sum;
    return before + s - x;
}
/* the smallest of x over the workgroup */
__device__ static inline uint64_t czs_min(uint64_t x) {
    __shared__ uint64_t wmin[CZS_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned d = 1; d < 64; d <<= 1) { const uint64_t y = czs_shfl_up64(x, d); if (lane >= d && y < x) x = y; }
    if (lane == 63) wmin[wave] = x;
    __syncthreads();
    uint64_t m = wmin[0];
    for (uint32_t w = 1; w < CZS_WAVES; w++) if (wmin[w] < m) m = wmin[w];
    __syncthreads();
    return m;
}
__device__ static inline uint32_t czs_ld32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }   /* (unaligned) */

__global__ void __launch_bounds__(CZS_THREADS) cz_seekable_plan_kernel(const cz_compress_result* results, uint32_t n, uint32_t flags,
                                                                       uint64_t stream_cap, unsigned long long* plan, cz_seekable_info* info) {
    const uint32_t t = threadIdx.x, cks = flags & 1u;
    uint64_t base = 0, content = 0, bad = ~0ull;
    /* A tile is CZS_ITEMS rows of CZS_THREADS records.  The records are read and the offsets written a row at a time (neighbouring
       lanes, neighbouring records: one workgroup has to stream all of them, and thread-sized pieces read at a third of this rate);
       in between the tile is turned in LDS so that a thread sums CZS_ITEMS consecutive sizes and the workgroup scans once. */
    __shared__ uint64_t turn[CZS_THREADS * CZS_ITEMS];
    for (uint64_t tile = 0; tile < n; tile += CZS_THREADS * CZS_ITEMS) {
        cz_compress_result r[CZS_ITEMS];
        for (uint32_t k = 0; k < CZS_ITEMS; k++) { const uint64_t i = tile + k * CZS_THREADS + t; r[k] = results[i < n ? i : n - 1]; }   /* (all loads in flight together) */
        for (uint32_t k = 0; k < CZS_ITEMS; k++) {
            const uint64_t i = tile + k * CZS_THREADS + t;
            uint64_t w = 0;
            if (i < n) {
                if (r[k].status != CZ_OK || (r[k].bytes_written >> 32) || (r[k].bytes_read >> 32) || (cks && !(r[k].flags & CZ_COMPRESS_CHECKSUM))) { if (i < bad) bad = i; }
                else { w = r[k].bytes_written; content += r[k].bytes_read; }
            }
            turn[k * CZS_THREADS + t] = w;
        }
        __syncthreads();
        uint64_t sum = 0, all;
        for (uint32_t k = 0; k < CZS_ITEMS; k++) sum += turn[t * CZS_ITEMS + k];
        uint64_t at = base + czs_scan(sum, &all);
        for (uint32_t k = 0; k < CZS_ITEMS; k++) { const uint64_t w = turn[t * CZS_ITEMS + k]; turn[t * CZS_ITEMS + k] = at; at += w; }
        __syncthreads();
        for (uint32_t k = 0; k < CZS_ITEMS; k++) { const uint64_t i = tile + k * CZS_THREADS + t; if (i < n) plan[i] = turn[k * CZS_THREADS + t]; }
        __syncthreads();                                                /* turn[] is written again */
        base += all;
    }
    uint64_t total;
    (void)czs_scan(content, &total);
    bad = czs_min(bad);
    if (t == 0) {
        const uint64_t need = base + 8 + (uint64_t)n * (cks ? 12u : 8u) + 9;
        const int status = bad != ~0ull ? CZ_E_INVALID_ARG : need > stream_cap ? CZ_E_OUTPUT_TOO_SMALL : CZ_OK;
        const uint32_t ok = bad == ~0ull;
        plan[n] = base; plan[n + 1] = status == CZ_OK;
        info->status = status; info->reason = 0; info->frames = n;
        info->frames_bytes = ok ? base : 0; info->content_bytes = ok ? total : 0; info->stream_bytes = ok ? need : 0;
        info->detail = ok ? 0 : bad; info->has_checksums = cks; info->reserved = 0;
    }
}

struct cz_seekable_gather_args {
    const uint8_t* frames_base; const uint64_t* frame_off; const cz_compress_result* results; const unsigned long long* plan;
    uint8_t* stream; uint32_t n, flags;
};
/* the last f in [lo, hi] with plan[f] <= p (plan[lo] <= p) */
__device__ static inline uint32_t czs_find(const unsigned long long* plan, uint32_t lo, uint32_t hi, uint64_t p) {
    while (lo < hi) { const uint32_t mid = lo + (hi - lo + 1) / 2; if (plan[mid] <= p) lo = mid; else hi = mid - 1; }
    return lo;
}
/* 32-bit word k of the table in front of the descriptor byte: magic, Frame_Size, the entries' fields, Number_Of_Frames */
__device__ static inline uint32_t czs_table_word(const cz_seekable_gather_args& a, uint32_t ew, uint64_t k) {
    if (k == 0) return CZS_SKIP_MAGIC_D;
    if (k == 1) return a.n * (4u * ew) + 9u;
    const uint64_t e = (k - 2) / ew; const uint32_t fld = (uint32_t)((k - 2) - e * ew);
    if (e >= a.n) return a.n;
    const cz_compress_result* r = a.results + e;
    return fld == 0 ? (uint32_t)r->bytes_written : fld == 1 ? (uint32_t)r->bytes_read : r->checksum;
}

__global__ void __launch_bounds__(CZS_THREADS) cz_seekable_gather_kernel(cz_seekable_gather_args a) {
    __shared__ uint32_t edge[2];
    const unsigned long long* plan = a.plan;
    if (!plan[a.n + 1]) return;                                         /* the plan said no: nothing is touched */
    const uint32_t t = threadIdx.x, ew = (a.flags & 1u) ? 3u : 2u;
    const uint64_t frames_bytes = plan[a.n], words = 2 + (uint64_t)a.n * ew + 1, total = frames_bytes + 4 * words + 5;
    const uint32_t mis = (uint32_t)((uintptr_t)a.stream & 15u);
    uint8_t* const vec0 = a.stream - mis;                               /* 16-byte aligned; vector v is vec0 + 16 v */
    const uint64_t vecs = (mis + total + 15) / 16, tiles = (vecs + CZS_TILE_VECS - 1) / CZS_TILE_VECS;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t v0 = tile * CZS_TILE_VECS, v1 = v0 + CZS_TILE_VECS < vecs ? v0 + CZS_TILE_VECS : vecs;
        /* stream positions of the tile: [p0, p1); the frames of its first and last frame byte, found by two waves side by side */
        const uint64_t p0 = v0 * 16 > mis ? v0 * 16 - mis : 0, p1 = v1 * 16 - mis < total ? v1 * 16 - mis : total;
        if (p0 < frames_bytes && (t == 0 || t == 64)) {
            const uint64_t p = t == 0 ? p0 : (p1 < frames_bytes ? p1 : frames_bytes) - 1;
            edge[t >> 6] = czs_find(plan, 0, a.n - 1, p);
        }
        __syncthreads();
        const uint32_t flo = edge[0], fhi = edge[1];
        for (uint64_t v = v0 + t; v < v1; v += CZS_THREADS) {
            const uint64_t b0 = v * 16, q0 = b0 > mis ? b0 - mis : 0, q1 = b0 + 16 - mis < total ? b0 + 16 - mis : total;   /* [q0, q1) */
            uint8_t* dst = vec0 + b0;
            uint32_t f = 0; uint64_t fs = 0, fe = 0;
            if (q0 < frames_bytes) { f = czs_find(plan, flo, fhi, q0); fs = plan[f]; fe = plan[f + 1]; }
            if (q1 - q0 == 16 && q1 <= fe) {                            /* a whole vector inside frame f */
                uint4 x; memcpy(&x, a.frames_base + a.frame_off[f] + (q0 - fs), 16);
                *(uint4*)dst = x;
                continue;
            }
            /* byte by byte (measured against putting the vector together in registers for one store: that takes 104 registers for
               40, halves the waves per SIMD and was 4 % and 12 % slower on the two batches of DESIGN.md §11) */
            uint64_t wk = ~0ull; uint32_t word = 0;
            for (uint64_t q = q0; q < q1; q++) {
                uint8_t byte;
                if (q < frames_bytes) {
                    while (q >= fe) { f++; fs = fe; fe = plan[f + 1]; }
                    byte = a.frames_base[a.frame_off[f] + (q - fs)];
                } else {
                    const uint64_t r = q - frames_bytes, k = r >> 2;
                    if (k < words) { if (k != wk) { wk = k; word = czs_table_word(a, ew, k); } byte = (uint8_t)(word >> (8 * (r & 3))); }
                    else if (r == 4 * words) byte = (uint8_t)((a.flags & 1u) << 7);
                    else byte = (uint8_t)(CZS_SEEK_MAGIC_D >> (8 * (r - 4 * words - 1)));
                }
                dst[q + mis - b0] = byte;
            }
        }
        __syncthreads();                                                /* edge[] is written again */
    }
}

struct cz_seekable_open_args {
    const uint8_t* stream; uint64_t stream_len, first, count; uint32_t out_align;
    uint64_t* in_off; uint64_t* in_len; uint64_t* out_off; uint64_t* out_cap; uint32_t* checksum; cz_seekable_info* info;
};
__global__ void __launch_bounds__(CZS_THREADS) cz_seekable_open_kernel(cz_seekable_open_args a) {
    __shared__ uint32_t head[4];                                        /* reason, Number_Of_Frames, entry size */
    const uint32_t t = threadIdx.x;
    const uint8_t* s = a.stream; const uint64_t len = a.stream_len;
    if (t == 0) {
        uint32_t reason = 0, n = 0, E = 8;
        if (len < 17) reason = 1;
        else if (czs_ld32(s + len - 4) != CZS_SEEK_MAGIC_D) reason = 2;
        else {
            const uint32_t desc = s[len - 5];
            n = czs_ld32(s + len - 9); E = (desc & 0x80u) ? 12u : 8u;
            if (desc & 0x7Cu) reason = 3;
            else if (n > CZS_MAX_FRAMES || 17 + (uint64_t)n * E > len) reason = 4;
            else {
                const uint64_t table = len - (17 + (uint64_t)n * E);
                if (czs_ld32(s + table) != CZS_SKIP_MAGIC_D || czs_ld32(s + table + 4) != n * E + 9u) reason = 5;
            }
        }
        head[0] = reason; head[1] = n; head[2] = E;
    }
    __syncthreads();
    uint32_t reason = cz_uni(head[0]);
    const uint32_t E = cz_uni(head[2]); const uint64_t n = cz_uni(head[1]);
    uint64_t comp = 0, content = 0, at = 0;
    const uint64_t table = reason ? 0 : len - (17 + n * E);
    const uint8_t* ent = reason ? s : s + table + 8;
    if (!reason) {
        /* both size columns, and the compressed sizes in front of the range */
        uint64_t c = 0, d = 0, b = 0;
        for (uint64_t i = t; i < n; i += CZS_THREADS) {
            const uint32_t x = czs_ld32(ent + i * E);
            c += x; d += czs_ld32(ent + i * E + 4); if (i < a.first) b += x;
        }
        (void)czs_scan(c, &comp); (void)czs_scan(d, &content); (void)czs_scan(b, &at);
        if (comp != table) reason = 6;
    }
    cz_seekable_info out;
    out.status = reason ? CZ_E_SEEK_TABLE : CZ_OK; out.reason = reason; out.frames = 0; out.frames_bytes = 0; out.content_bytes = 0;
    out.stream_bytes = 0; out.detail = 0; out.has_checksums = 0; out.reserved = 0;
    if (reason) { if (t == 0) *a.info = out; return; }
    out.frames = n; out.frames_bytes = comp; out.content_bytes = content; out.stream_bytes = len; out.has_checksums = E == 12;
    uint64_t count = a.count;
    if (a.first <= n && count == ~0ull) count = n - a.first;
    if (a.first > n || count > n - a.first) { out.status = CZ_E_INVALID_ARG; if (t == 0) *a.info = out; return; }
    const uint64_t align = a.out_align;
    uint64_t pos = 0, need = 0;
    for (uint64_t tile = 0; tile < count; tile += CZS_THREADS * CZS_ITEMS) {
        const uint64_t i0 = tile + (uint64_t)t * CZS_ITEMS;
        uint32_t c[CZS_ITEMS], d[CZS_ITEMS]; uint64_t csum = 0, psum = 0;
        for (uint32_t k = 0; k < CZS_ITEMS; k++) {                      /* (all loads in flight together) */
            const uint8_t* e = ent + (a.first + (i0 + k < count ? i0 + k : count - 1)) * E;
            c[k] = czs_ld32(e); d[k] = czs_ld32(e + 4);
        }
        for (uint32_t k = 0; k < CZS_ITEMS; k++) {
            if (i0 + k >= count) { c[k] = 0; d[k] = 0; }
            csum += c[k]; psum += ((uint64_t)d[k] + align - 1) & ~(align - 1);
        }
        uint64_t call, pall;
        uint64_t ci = at + czs_scan(csum, &call), po = pos + czs_scan(psum, &pall);
        for (uint32_t k = 0; k < CZS_ITEMS; k++) {
            const uint64_t i = i0 + k;
            if (i < count) {
                if (a.in_off) a.in_off[i] = ci;
                if (a.in_len) a.in_len[i] = c[k];
                if (a.out_off) a.out_off[i] = po;
                if (a.out_cap) a.out_cap[i] = d[k];
                if (a.checksum) a.checksum[i] = E == 12 ? czs_ld32(ent + (a.first + i) * E + 8) : 0u;
                if (i + 1 == count) need = po + d[k];
            }
            ci += c[k]; po += ((uint64_t)d[k] + align - 1) & ~(align - 1);
        }
        at += call; pos += pall;
    }
    (void)czs_scan(need, &need);                                        /* (one thread holds it) */
    out.detail = need;
    if (t == 0) *a.info = out;
}
