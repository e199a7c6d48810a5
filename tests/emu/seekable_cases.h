/*
 * TEST INFRASTRUCTURE ONLY — the case file that seekable_host_main.cpp (cz_seekable_*_host) and emu_seekable.cpp (the kernels) both
 * read, and the result file both write, so that one Python test drives the two implementations with the same bytes.
 *   cases.bin : a sequence of
 *     'P' u32 flags, u32 dst_residue, u64 stream_cap, u64 n, n x { cz_compress_result, u64 data_len, data }
 *     'O' u32 src_residue, u64 stream_len, stream, u64 first, u64 count, u32 out_align, u64 k, u8 arrays
 *   result.bin: per case
 *     P: i32 return value, cz_seekable_info, u64 block_len = dst_residue + stream_cap, the whole block (0xEE where nothing was written)
 *     O: i32 return value, cz_seekable_info, u64 k, in_off[k], in_len[k], out_off[k], out_cap[k] (u64), checksum[k] (u32); 0xA5 where
 *        nothing was written (arrays 0: no arrays were passed, k entries of poison all the same)
 * The allocation discipline is what makes ASan useful.  Every frame sits in a heap block of its own that ENDS with the frame and
 * has i % 16 bytes of 0x5A in front of it, so the sources take every residue and a read past a frame's end is a report; the stream
 * of a pack is the last stream_cap bytes of a block with dst_residue bytes in front; the stream of an open ends its block; every
 * array is a block of exactly k entries.
 */
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "cairo_zstd_amd.h"

struct sk_pack_case {
    uint32_t flags = 0, residue = 0; uint64_t cap = 0, n = 0;
    std::vector<cz_compress_result> res; std::vector<uint8_t*> blocks; std::vector<uint64_t> off;
    const uint8_t* base = nullptr; uint8_t* block = nullptr; uint8_t* stream = nullptr;
    cz_compress_result* d_res = nullptr; uint64_t* d_off = nullptr;     /* exact-size copies */
};
struct sk_open_case {
    uint32_t residue = 0, align = 1; uint64_t len = 0, first = 0, count = 0, k = 0; uint8_t arrays = 0;
    uint8_t* block = nullptr; uint8_t* stream = nullptr;
    uint64_t* a[4] = {nullptr, nullptr, nullptr, nullptr}; uint32_t* sums = nullptr;
};

static bool sk_rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static bool sk_read_pack(FILE* f, sk_pack_case* c) {
    if (!sk_rd(f, &c->flags, 4) || !sk_rd(f, &c->residue, 4) || !sk_rd(f, &c->cap, 8) || !sk_rd(f, &c->n, 8)) return false;
    c->res.resize(c->n); c->blocks.resize(c->n); c->off.resize(c->n);
    std::vector<uint8_t*> data(c->n);
    uintptr_t lowest = ~(uintptr_t)0;
    for (uint64_t i = 0; i < c->n; i++) {
        uint64_t len;
        if (!sk_rd(f, &c->res[i], sizeof(cz_compress_result)) || !sk_rd(f, &len, 8)) return false;
        const size_t front = (size_t)(i % 16);
        c->blocks[i] = (uint8_t*)malloc(front + len); memset(c->blocks[i], 0x5A, front);
        data[i] = c->blocks[i] + front;
        if (!sk_rd(f, data[i], len)) return false;
        if ((uintptr_t)data[i] < lowest) lowest = (uintptr_t)data[i];
    }
    c->base = c->n ? (const uint8_t*)lowest : nullptr;
    for (uint64_t i = 0; i < c->n; i++) c->off[i] = (uint64_t)((uintptr_t)data[i] - lowest);
    c->d_res = (cz_compress_result*)malloc(c->n * sizeof(cz_compress_result)); c->d_off = (uint64_t*)malloc(c->n * 8);
    if (c->n) { memcpy(c->d_res, c->res.data(), c->n * sizeof(cz_compress_result)); memcpy(c->d_off, c->off.data(), c->n * 8); }
    c->block = (uint8_t*)malloc(c->residue + c->cap); memset(c->block, 0xEE, c->residue + c->cap);
    c->stream = c->block + c->residue;
    return true;
}
static void sk_write_pack(FILE* g, sk_pack_case* c, int ret, const cz_seekable_info* info) {
    const uint64_t bl = c->residue + c->cap;
    fwrite(&ret, 4, 1, g); fwrite(info, sizeof *info, 1, g); fwrite(&bl, 8, 1, g); fwrite(c->block, 1, bl, g);
    for (uint8_t* b : c->blocks) free(b);
    free(c->d_res); free(c->d_off); free(c->block);
}

static bool sk_read_open(FILE* f, sk_open_case* c) {
    if (!sk_rd(f, &c->residue, 4) || !sk_rd(f, &c->len, 8)) return false;
    c->block = (uint8_t*)malloc(c->residue + c->len); memset(c->block, 0x5A, c->residue);
    c->stream = c->block + c->residue;
    if (!sk_rd(f, c->stream, c->len)) return false;
    if (!sk_rd(f, &c->first, 8) || !sk_rd(f, &c->count, 8) || !sk_rd(f, &c->align, 4) || !sk_rd(f, &c->k, 8) || !sk_rd(f, &c->arrays, 1)) return false;
    for (int j = 0; j < 4; j++) { c->a[j] = (uint64_t*)malloc(c->k * 8); memset(c->a[j], 0xA5, c->k * 8); }
    c->sums = (uint32_t*)malloc(c->k * 4); memset(c->sums, 0xA5, c->k * 4);
    return true;
}
static void sk_write_open(FILE* g, sk_open_case* c, int ret, const cz_seekable_info* info) {
    fwrite(&ret, 4, 1, g); fwrite(info, sizeof *info, 1, g); fwrite(&c->k, 8, 1, g);
    for (int j = 0; j < 4; j++) { fwrite(c->a[j], 8, c->k, g); free(c->a[j]); }
    fwrite(c->sums, 4, c->k, g); free(c->sums); free(c->block);
}
