/*
 * czstd_seekable_host.h — seekable streams on the CPU: cz_seekable_bound, cz_seekable_pack_host, cz_seekable_open_host
 * (include/cairo_zstd_amd.h).  Plain C++, nothing from HIP: czstd_host.hip includes it for the library, and a
 * stand-alone program can compile it with any C++ compiler.  It is the library's second implementation of the format; the kernels
 * of czstd_seekable.hip are held to it.
 *
 *     frame 0 | ... | frame n-1 | 0x184D2A5E | Frame_Size = n * E + 9 | n x { Compressed_Size, Decompressed_Size, [Checksum] } |
 *     Number_Of_Frames | Seek_Table_Descriptor (1 byte) | 0x8F92EAB1          — 32-bit little-endian fields, nothing aligned
 */
#ifndef CZSTD_SEEKABLE_HOST_H
#define CZSTD_SEEKABLE_HOST_H
#include <stdint.h>
#include <string.h>

#include "cairo_zstd_amd.h"

#ifndef CZ_EXPORT
#define CZ_EXPORT extern "C"
#endif

#define CZS_SKIP_MAGIC 0x184D2A5Eu
#define CZS_SEEK_MAGIC 0x8F92EAB1u

static inline uint32_t czs_rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static inline void czs_wr32(uint8_t* p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i)); }

CZ_EXPORT uint64_t cz_seekable_bound(uint64_t frame_bytes, size_t n, uint32_t flags) {
    return frame_bytes + 8 + (uint64_t)n * ((flags & CZ_SEEKABLE_CHECKSUMS) ? 12u : 8u) + 9;
}

CZ_EXPORT int cz_seekable_pack_host(const void* frames_base, const uint64_t* frame_off, const cz_compress_result* results, size_t n,
                                    void* stream, uint64_t stream_cap, uint32_t flags, cz_seekable_info* info) {
    if (!info) return CZ_E_INVALID_ARG;
    memset(info, 0, sizeof *info);
    info->status = CZ_E_INVALID_ARG;
    if ((flags & ~CZ_SEEKABLE_CHECKSUMS) || n > CZ_SEEKABLE_MAX_FRAMES || !stream || (n && (!frames_base || !frame_off || !results))) return CZ_E_INVALID_ARG;
    const uint32_t cks = flags & CZ_SEEKABLE_CHECKSUMS, E = cks ? 12u : 8u;
    info->frames = n; info->has_checksums = cks;
    uint64_t comp = 0, content = 0;
    for (size_t i = 0; i < n; i++) {
        const cz_compress_result& r = results[i];
        if (r.status != CZ_OK || (r.bytes_written >> 32) || (r.bytes_read >> 32) || (cks && !(r.flags & CZ_COMPRESS_CHECKSUM))) { info->detail = i; return CZ_E_INVALID_ARG; }
        comp += r.bytes_written; content += r.bytes_read;
    }
    info->frames_bytes = comp; info->content_bytes = content; info->stream_bytes = cz_seekable_bound(comp, n, flags);
    if (info->stream_bytes > stream_cap) return info->status = CZ_E_OUTPUT_TOO_SMALL;
    uint8_t* out = (uint8_t*)stream;
    for (size_t i = 0; i < n; i++) {
        if (results[i].bytes_written) memcpy(out, (const uint8_t*)frames_base + frame_off[i], (size_t)results[i].bytes_written);
        out += results[i].bytes_written;
    }
    czs_wr32(out, CZS_SKIP_MAGIC); czs_wr32(out + 4, (uint32_t)(n * E + 9)); out += 8;
    for (size_t i = 0; i < n; i++, out += E) {
        czs_wr32(out, (uint32_t)results[i].bytes_written); czs_wr32(out + 4, (uint32_t)results[i].bytes_read);
        if (cks) czs_wr32(out + 8, results[i].checksum);
    }
    czs_wr32(out, (uint32_t)n); out[4] = (uint8_t)(cks ? 0x80 : 0); czs_wr32(out + 5, CZS_SEEK_MAGIC);
    return info->status = CZ_OK;
}

CZ_EXPORT int cz_seekable_open_host(const void* stream, uint64_t stream_len, uint64_t first, uint64_t count, uint32_t out_align,
                                    uint64_t* in_off, uint64_t* in_len, uint64_t* out_off, uint64_t* out_cap, uint32_t* checksum,
                                    cz_seekable_info* info) {
    if (!info) return CZ_E_INVALID_ARG;
    memset(info, 0, sizeof *info);
    info->status = CZ_E_INVALID_ARG;
    if (out_align == 0 || out_align > 4096 || (out_align & (out_align - 1)) || (!stream && stream_len)) return CZ_E_INVALID_ARG;
    const uint8_t* s = (const uint8_t*)stream;
    info->status = CZ_E_SEEK_TABLE;
    if (stream_len < 17) { info->reason = 1; return CZ_E_SEEK_TABLE; }
    if (czs_rd32(s + stream_len - 4) != CZS_SEEK_MAGIC) { info->reason = 2; return CZ_E_SEEK_TABLE; }
    const uint32_t desc = s[stream_len - 5];
    if (desc & 0x7Cu) { info->reason = 3; return CZ_E_SEEK_TABLE; }
    const uint64_t n = czs_rd32(s + stream_len - 9), E = (desc & 0x80u) ? 12u : 8u;
    if (n > CZ_SEEKABLE_MAX_FRAMES || 17 + n * E > stream_len) { info->reason = 4; return CZ_E_SEEK_TABLE; }
    const uint64_t table = stream_len - (17 + n * E);
    if (czs_rd32(s + table) != CZS_SKIP_MAGIC || czs_rd32(s + table + 4) != (uint32_t)(n * E + 9)) { info->reason = 5; return CZ_E_SEEK_TABLE; }
    const uint8_t* ent = s + table + 8;
    uint64_t comp = 0, content = 0;
    for (uint64_t i = 0; i < n; i++) { comp += czs_rd32(ent + i * E); content += czs_rd32(ent + i * E + 4); }
    if (comp != table) { info->reason = 6; return CZ_E_SEEK_TABLE; }
    info->frames = n; info->frames_bytes = comp; info->content_bytes = content; info->stream_bytes = stream_len;
    info->has_checksums = desc >> 7;
    if (first > n) return info->status = CZ_E_INVALID_ARG;
    if (count == UINT64_MAX) count = n - first;
    if (count > n - first) return info->status = CZ_E_INVALID_ARG;
    uint64_t at = 0, out = 0, need = 0;
    for (uint64_t i = 0; i < first; i++) at += czs_rd32(ent + i * E);
    for (uint64_t i = 0; i < count; i++) {
        const uint8_t* e = ent + (first + i) * E;
        const uint64_t c = czs_rd32(e), d = czs_rd32(e + 4);
        if (in_off) in_off[i] = at;
        if (in_len) in_len[i] = c;
        if (out_off) out_off[i] = out;
        if (out_cap) out_cap[i] = d;
        if (checksum) checksum[i] = E == 12 ? czs_rd32(e + 8) : 0u;
        need = out + d;
        at += c; out += (d + out_align - 1) & ~(uint64_t)(out_align - 1);
    }
    info->detail = need;
    return info->status = CZ_OK;
}
#endif /* CZSTD_SEEKABLE_HOST_H */
