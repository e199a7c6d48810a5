/*
 * czstd_seekable_read_host.h — byte ranges out of a seekable stream on the CPU: cz_seekable_locate_host, cz_seekable_gather_host
 * (include/cairo_zstd_amd.h).  Plain C++, nothing from HIP: czstd_host.hip includes it for the library, and a
 * stand-alone program can compile it with any C++ compiler.  It is the library's second implementation of locate and gather; the
 * kernels of czstd_seekable_read.hip are held to it.  It does not work the way they do: the frames of a range come from
 * std::upper_bound over the scanned sizes, the selection from a difference array over the frames, the gather from one memcpy per
 * piece.
 */
#ifndef CZSTD_SEEKABLE_READ_HOST_H
#define CZSTD_SEEKABLE_READ_HOST_H
#include <algorithm>
#include <new>
#include <vector>

#include "czstd_seekable_host.h"

CZ_EXPORT int cz_seekable_locate_host(const void* stream, uint64_t stream_len, const uint64_t* range_off, const uint64_t* range_len, size_t m,
                                      uint32_t out_align, uint64_t frames_cap,
                                      uint32_t* frame, uint64_t* in_off, uint64_t* in_len, uint64_t* out_off, uint64_t* out_cap,
                                      uint32_t* checksum, uint64_t* content_off, cz_seekable_span* spans, cz_seekable_read_info* info) try {
    if (!info) return CZ_E_INVALID_ARG;
    memset(info, 0, sizeof *info);
    info->status = CZ_E_INVALID_ARG;
    if (m > CZ_SEEKABLE_MAX_FRAMES || (m && (!range_off || !range_len))) return CZ_E_INVALID_ARG;
    cz_seekable_info table;
    const int st = cz_seekable_open_host(stream, stream_len, 0, 0, out_align, nullptr, nullptr, nullptr, nullptr, nullptr, &table);
    if (st == CZ_E_SEEK_TABLE) { info->reason = table.reason; return info->status = st; }
    if (st != CZ_OK) return CZ_E_INVALID_ARG;                           /* out_align, a NULL stream */
    const uint64_t n = table.frames, E = table.has_checksums ? 12u : 8u, content = table.content_bytes, align = out_align;
    const uint8_t* ent = (const uint8_t*)stream + table.frames_bytes + 8;
    info->frames = n; info->content_bytes = content; info->has_checksums = table.has_checksums;
    for (size_t j = 0; j < m; j++)
        if (range_off[j] > content || range_len[j] > content - range_off[j]) { info->detail = j; return CZ_E_INVALID_ARG; }
    std::vector<uint64_t> start(n + 1), comp(n + 1);
    for (uint64_t i = 0; i < n; i++) { comp[i + 1] = comp[i] + czs_rd32(ent + i * E); start[i + 1] = start[i] + czs_rd32(ent + i * E + 4); }
    /* touched[i]: ranges that begin in or in front of frame i and end in or behind it */
    std::vector<int64_t> diff(n + 1, 0);
    std::vector<uint64_t> first(m), last(m);
    uint64_t dst = 0;
    for (size_t j = 0; j < m; j++) {
        dst += range_len[j];
        if (!range_len[j]) continue;
        first[j] = (uint64_t)(std::upper_bound(start.begin(), start.begin() + n, range_off[j]) - start.begin()) - 1;
        last[j] = (uint64_t)(std::upper_bound(start.begin(), start.begin() + n, range_off[j] + (range_len[j] - 1)) - start.begin()) - 1;
        diff[first[j]]++; diff[last[j] + 1]--;
    }
    std::vector<uint64_t> rank(n), sel_out;
    std::vector<uint64_t> sel;
    uint64_t pos = 0, need = 0; int64_t touched = 0;
    for (uint64_t i = 0; i < n; i++) {
        touched += diff[i];
        const uint64_t d = start[i + 1] - start[i];
        rank[i] = sel.size();
        if (touched > 0 && d) { sel.push_back(i); sel_out.push_back(pos); need = pos + d; pos += (d + align - 1) & ~(align - 1); }
    }
    const uint64_t k = sel.size();
    info->selected = k; info->out_bytes = need; info->dst_bytes = dst;
    if ((frame || in_off || in_len || out_off || out_cap || checksum || content_off) && k > frames_cap) return info->status = CZ_E_OUTPUT_TOO_SMALL;
    for (uint64_t s = 0; s < k; s++) {
        const uint64_t i = sel[s];
        if (frame) frame[s] = (uint32_t)i;
        if (in_off) in_off[s] = comp[i];
        if (in_len) in_len[s] = comp[i + 1] - comp[i];
        if (out_off) out_off[s] = sel_out[s];
        if (out_cap) out_cap[s] = start[i + 1] - start[i];
        if (checksum) checksum[s] = E == 12 ? czs_rd32(ent + i * E + 8) : 0u;
        if (content_off) content_off[s] = start[i];
    }
    if (spans) {
        uint64_t at = 0;
        for (size_t j = 0; j < m; j++) {
            cz_seekable_span sp; sp.dst_off = at; sp.src_off = 0; sp.sel_first = 0; sp.sel_count = 0;
            if (range_len[j]) {
                sp.sel_first = (uint32_t)rank[first[j]]; sp.sel_count = (uint32_t)(rank[last[j]] - rank[first[j]] + 1);
                sp.src_off = sel_out[sp.sel_first] + (range_off[j] - start[first[j]]);
            }
            spans[j] = sp;
            at += range_len[j];
        }
    }
    return info->status = CZ_OK;
} catch (const std::bad_alloc&) { return info->status = CZ_E_OUT_OF_MEMORY; }

CZ_EXPORT int cz_seekable_gather_host(const void* decoded, const uint64_t* out_off, const uint64_t* content_off, uint64_t k,
                                      const uint64_t* range_off, const uint64_t* range_len, const cz_seekable_span* spans, size_t m,
                                      void* dst, uint64_t dst_bytes) {
    if (m > CZ_SEEKABLE_MAX_FRAMES) return CZ_E_INVALID_ARG;
    if (m == 0 || dst_bytes == 0) return CZ_OK;
    if (!decoded || !out_off || !content_off || !k || !range_off || !range_len || !spans || !dst) return CZ_E_INVALID_ARG;
    for (size_t j = 0; j < m; j++) {
        const cz_seekable_span& sp = spans[j];
        uint64_t left = range_len[j], c = range_off[j], s = sp.sel_first;
        if (!left) continue;
        if (sp.dst_off > dst_bytes || left > dst_bytes - sp.dst_off || s >= k || sp.sel_count > k - s) return CZ_E_INVALID_ARG;
        const uint64_t end = s + sp.sel_count;
        uint8_t* to = (uint8_t*)dst + sp.dst_off;
        while (left) {
            while (s + 1 < end && content_off[s + 1] <= c) s++;         /* the selected frame that holds content byte c */
            const uint64_t stop = s + 1 < end ? content_off[s + 1] : c + left, take = left < stop - c ? left : stop - c;
            memcpy(to, (const uint8_t*)decoded + out_off[s] + (c - content_off[s]), (size_t)take);
            to += take; c += take; left -= take;
        }
    }
    return CZ_OK;
}
#endif /* CZSTD_SEEKABLE_READ_HOST_H */
