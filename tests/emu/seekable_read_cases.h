/*
 * TEST INFRASTRUCTURE ONLY — the case file that seekable_read_host_main.cpp (cz_seekable_locate_host, cz_seekable_gather_host) and
 * emu_seekable_read.cpp (the kernels of czstd_seekable_read.hip) both read, and the result file both write, so that one Python test
 * drives the two implementations with the same bytes.
 *   cases.bin : a sequence of
 *     'L' u64 stream_len, stream, u32 calls, calls x { u64 m, off[m], len[m] (u64), u32 out_align, u64 frames_cap, u64 k, u8 arrays }
 *         one index of the stream and `calls` locates on it, one after another (the host function is stateless: it parses each time)
 *     'G' u32 dst_residue, u64 k, out_off[k], content_off[k] (u64), u64 decoded_len, decoded, u64 m, off[m], len[m] (u64),
 *         spans[m] (24 bytes each), u64 dst_bytes
 *   result.bin: per case
 *     L: i32 return value of the index, cz_seekable_info; when that is CZ_OK per call: i32 return value, cz_seekable_read_info, u8 clean
 *        (the per-frame scratch and the bad-range word were all 0 after the call; the host program writes 1), u64 k, frame[k] (u32),
 *        in_off[k], in_len[k], out_off[k], out_cap[k] (u64), checksum[k] (u32), content_off[k] (u64), u64 m, spans[m]; 0xA5 where
 *        nothing was written (arrays 0: no arrays were passed, k and m entries of poison all the same)
 *     G: i32 return value, u64 block_len = dst_residue + dst_bytes, the whole block (0xEE where nothing was written)
 * The allocation discipline is what makes ASan useful: the stream ends its block, every array, the scratch, the decoded buffer and
 * the destination (dst_residue bytes into a block that ends with it) are heap blocks of their exact size.
 */
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "cairo_zstd_amd.h"

template <class T> static T* sr_block(uint64_t count, int fill) {
    T* p = (T*)malloc(count * sizeof(T)); memset(p, fill, count * sizeof(T));
    return p;
}
static bool sr_rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

struct sr_call {
    uint64_t m = 0, frames_cap = 0, k = 0; uint32_t align = 1; uint8_t arrays = 0;
    uint64_t* off = nullptr; uint64_t* len = nullptr;
    uint32_t* frame = nullptr; uint64_t* a[4] = {nullptr, nullptr, nullptr, nullptr}; uint32_t* sums = nullptr; uint64_t* content_off = nullptr;
    cz_seekable_span* spans = nullptr;
};
static bool sr_read_call(FILE* f, sr_call* c) {
    if (!sr_rd(f, &c->m, 8)) return false;
    c->off = sr_block<uint64_t>(c->m, 0); c->len = sr_block<uint64_t>(c->m, 0);
    if (!sr_rd(f, c->off, c->m * 8) || !sr_rd(f, c->len, c->m * 8)) return false;
    if (!sr_rd(f, &c->align, 4) || !sr_rd(f, &c->frames_cap, 8) || !sr_rd(f, &c->k, 8) || !sr_rd(f, &c->arrays, 1)) return false;
    c->frame = sr_block<uint32_t>(c->k, 0xA5); c->sums = sr_block<uint32_t>(c->k, 0xA5); c->content_off = sr_block<uint64_t>(c->k, 0xA5);
    for (int j = 0; j < 4; j++) c->a[j] = sr_block<uint64_t>(c->k, 0xA5);
    c->spans = sr_block<cz_seekable_span>(c->m, 0xA5);
    return true;
}
static void sr_write_call(FILE* g, sr_call* c, int ret, const cz_seekable_read_info* info, uint8_t clean) {
    fwrite(&ret, 4, 1, g); fwrite(info, sizeof *info, 1, g); fwrite(&clean, 1, 1, g); fwrite(&c->k, 8, 1, g);
    fwrite(c->frame, 4, c->k, g);
    for (int j = 0; j < 4; j++) fwrite(c->a[j], 8, c->k, g);
    fwrite(c->sums, 4, c->k, g); fwrite(c->content_off, 8, c->k, g);
    fwrite(&c->m, 8, 1, g); fwrite(c->spans, sizeof(cz_seekable_span), c->m, g);
    free(c->off); free(c->len); free(c->frame); free(c->sums); free(c->content_off); free(c->spans);
    for (int j = 0; j < 4; j++) free(c->a[j]);
}

struct sr_stream { uint64_t len = 0; uint8_t* bytes = nullptr; uint32_t calls = 0; };
static bool sr_read_stream(FILE* f, sr_stream* s) {
    if (!sr_rd(f, &s->len, 8)) return false;
    s->bytes = sr_block<uint8_t>(s->len, 0);
    return sr_rd(f, s->bytes, s->len) && sr_rd(f, &s->calls, 4);
}

struct sr_gather_case {
    uint32_t residue = 0; uint64_t k = 0, decoded_len = 0, m = 0, dst_bytes = 0;
    uint64_t* out_off = nullptr; uint64_t* content_off = nullptr; uint8_t* decoded = nullptr;
    uint64_t* off = nullptr; uint64_t* len = nullptr; cz_seekable_span* spans = nullptr; uint8_t* block = nullptr; uint8_t* dst = nullptr;
};
static bool sr_read_gather(FILE* f, sr_gather_case* c) {
    if (!sr_rd(f, &c->residue, 4) || !sr_rd(f, &c->k, 8)) return false;
    c->out_off = sr_block<uint64_t>(c->k, 0); c->content_off = sr_block<uint64_t>(c->k, 0);
    if (!sr_rd(f, c->out_off, c->k * 8) || !sr_rd(f, c->content_off, c->k * 8) || !sr_rd(f, &c->decoded_len, 8)) return false;
    c->decoded = sr_block<uint8_t>(c->decoded_len, 0);
    if (!sr_rd(f, c->decoded, c->decoded_len) || !sr_rd(f, &c->m, 8)) return false;
    c->off = sr_block<uint64_t>(c->m, 0); c->len = sr_block<uint64_t>(c->m, 0); c->spans = sr_block<cz_seekable_span>(c->m, 0);
    if (!sr_rd(f, c->off, c->m * 8) || !sr_rd(f, c->len, c->m * 8) || !sr_rd(f, c->spans, c->m * sizeof(cz_seekable_span))) return false;
    if (!sr_rd(f, &c->dst_bytes, 8)) return false;
    c->block = sr_block<uint8_t>(c->residue + c->dst_bytes, 0xEE); c->dst = c->block + c->residue;
    return true;
}
static void sr_write_gather(FILE* g, sr_gather_case* c, int ret) {
    const uint64_t bl = c->residue + c->dst_bytes;
    fwrite(&ret, 4, 1, g); fwrite(&bl, 8, 1, g); fwrite(c->block, 1, bl, g);
    free(c->out_off); free(c->content_off); free(c->decoded); free(c->off); free(c->len); free(c->spans); free(c->block);
}
