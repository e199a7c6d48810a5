/*
 * TEST INFRASTRUCTURE ONLY — runs the batch path of cz_context_set_dictionaries (the unmodified kernel source) on the CPU through
 * tests/emu/hip/hip_runtime.h, under ASan+UBSan: the dictionaries parsed by cz_dict_setup_kernel, the table filled as the host
 * library fills it (sorted by ID), then [cz_scan_kernel (two passes), cz_chain_kernel, cz_huf1_kernel / cz_huf_kernel,
 * cz_tile_kernel (EMU_CHAIN / EMU_LIT),] cz_decode_frames_kernel.
 * usage: emu_multidict <batch.bin> <result.bin>
 *   batch.bin : u64 n, then n x { u64 in_len, u64 out_cap, in bytes }
 *   result.bin: n x { cz_frame_result, out bytes (bytes_produced) }
 * EMU_DICTS=<file>[:<file>...]  the registered dictionaries;  EMU_NOID_DICT=<file>  the no-ID dictionary (optional)
 * Output regions start as 0xEE: a frame that writes nothing leaves them so (the runner reads them back with EMU_DUMP_ALL=1).
 */
#include "emu_harness.h"
#include <algorithm>
#include <string>

#include "czstd_kernels.hip"
#include "czstd_chain.hip"
#include "czstd_pre.hip"
#include "czstd_dict.h"

/* one dictionary as cz_dictionary_decode makes it: exact-size copy of the bytes, the state cz_dict_setup_kernel builds, its entry */
static int load_dict(const char* path, cz_dict_entry* e) {
    FILE* df = fopen(path, "rb"); if (!df) return 2;
    fseek(df, 0, SEEK_END); long dl = ftell(df); fseek(df, 0, SEEK_SET);
    uint8_t* raw = (uint8_t*)malloc(dl ? (size_t)dl : 1);
    if (dl && fread(raw, 1, (size_t)dl, df) != (size_t)dl) return 2;
    fclose(df);
    cz_device_frame_state* st = (cz_device_frame_state*)calloc(1, sizeof(cz_device_frame_state));
    uint64_t res[4] = {0, 0, 0, 0};
    emu_launch(1, 64, [&] { cz_dict_setup_kernel(raw, (uint64_t)dl, st, res); });
    fprintf(stderr, "EMU_DICT %s: status %llu content offset %llu id %llu\n", path, (unsigned long long)res[0], (unsigned long long)res[1], (unsigned long long)res[2]);
    if (res[0]) return 3;
    e->id = (uint32_t)res[2]; e->pad = 0; e->state = st; e->content = raw + res[1]; e->content_len = (uint64_t)dl - res[1];
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    uint64_t n; if (fread(&n, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> in_off(n), in_len(n), out_off(n), out_cap(n);
    std::vector<uint8_t> in; uint64_t out_total = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t l, c; if (fread(&l, 8, 1, f) != 1 || fread(&c, 8, 1, f) != 1) return 2;
        in_off[i] = in.size(); in_len[i] = l; out_cap[i] = c; out_off[i] = out_total; out_total += c;
        size_t at = in.size(); in.resize(at + l);
        if (l && fread(in.data() + at, 1, l, f) != l) return 2;
    }
    fclose(f);
    /* exact-size heap blocks so that ASan sees any byte read or written out of range */
    uint8_t* in_exact = (uint8_t*)malloc(in.size() ? in.size() : 1); if (in.size()) memcpy(in_exact, in.data(), in.size());
    uint8_t* out = (uint8_t*)malloc(out_total ? out_total : 1); memset(out, 0xEE, out_total);
    std::vector<cz_frame_result> res(n);
    memset(res.data(), 0xA5, n * sizeof(cz_frame_result));            /* a record nobody writes shows up */
    uint32_t counter = 0;
    const int grid = 2;
    uint8_t* lit = (uint8_t*)malloc((size_t)grid * CZ_WG_SCRATCH_BYTES);
    cz_batch_args a; memset(&a, 0, sizeof a);
    a.in_base = in_exact; a.in_off = in_off.data(); a.in_len = in_len.data();
    a.out_base = out; a.out_off = out_off.data(); a.out_cap = out_cap.data();
    a.results = res.data(); a.tasks = nullptr; a.n = (uint32_t)n; a.work_counter = &counter;
    a.lit_scratch = lit; a.lit_scratch_stride = CZ_WG_SCRATCH_BYTES; a.verify_checksum = getenv("EMU_VERIFY") ? (uint32_t)atoi(getenv("EMU_VERIFY")) : 1u;
    /* the table, as cz_context_set_dictionaries fills it: sorted by ID, and always at least one entry */
    std::vector<cz_dict_entry> table;
    if (const char* ds = getenv("EMU_DICTS")) {
        std::string all(ds);
        for (size_t at = 0; at <= all.size();) {
            size_t end = all.find(':', at); if (end == std::string::npos) end = all.size();
            if (end > at) { cz_dict_entry e; const int st = load_dict(all.substr(at, end - at).c_str(), &e); if (st) return st; table.push_back(e); }
            at = end + 1;
        }
    }
    std::sort(table.begin(), table.end(), [](const cz_dict_entry& x, const cz_dict_entry& y) { return x.id < y.id; });
    const uint32_t ndicts = (uint32_t)table.size();
    cz_dict_entry* dicts = (cz_dict_entry*)malloc((ndicts ? ndicts : 1) * sizeof(cz_dict_entry));   /* exact size: a lookup out of range is an ASan report */
    if (ndicts) memcpy(dicts, table.data(), ndicts * sizeof(cz_dict_entry));
    a.dicts = dicts; a.ndicts = ndicts;
    if (const char* nd = getenv("EMU_NOID_DICT")) {
        cz_dict_entry e; const int st = load_dict(nd, &e); if (st) return st;
        a.dict_state = e.state; a.dict = e.content; a.dict_len = e.content_len;
    }
    /* EMU_CHAIN=<bytes>: the FSE-chain pre-pass with an arena of that many bytes; EMU_LIT=<bytes>: the literal / copy half too */
    const char* ce = getenv("EMU_CHAIN");
    unsigned long long chain_top[8] = {0, 0, 0, 0, 0, 0, 0, 0}; uint32_t chain_counter = 0;
    std::vector<uint64_t> frame_first(n ? n : 1, 0);
    uint64_t* arena = nullptr;
    if (ce && atoll(ce) > 0) {
        size_t bytes = (size_t)atoll(ce);
        arena = (uint64_t*)malloc(bytes); a.chain_arena = arena; a.chain_capacity = bytes / 8; a.chain_top = chain_top;
        a.frame_first = frame_first.data(); a.chain_counter = &chain_counter;
    }
    unsigned long long lit_top[4] = {0, 0, 0, 0}; std::vector<uint64_t> lit_first(n ? n : 1, 0); uint8_t* lit_arena = nullptr;
    const size_t lit_bytes = arena && getenv("EMU_LIT") ? (size_t)atoll(getenv("EMU_LIT")) : 0;
    std::vector<cz_lit_seg> lit_segs; std::vector<cz_copy_seg> copy_segs; std::vector<uint32_t> frame_pre(n ? n : 1, 0);
    if (lit_bytes) {
        lit_arena = (uint8_t*)malloc(lit_bytes); a.lit_arena = lit_arena; a.lit_capacity = lit_bytes; a.lit_top = lit_top; a.lit_first = lit_first.data();
        const size_t cap = lit_bytes / 256 + 4096;
        lit_segs.resize(cap); copy_segs.resize(cap);
        a.lit_segs = lit_segs.data(); a.lit_seg_capacity = (uint32_t)cap; a.copy_segs = copy_segs.data(); a.copy_seg_capacity = (uint32_t)cap; a.frame_pre = frame_pre.data();
    }
    std::vector<cz_blk_desc> blk_desc; std::vector<uint32_t> scan_ctl(CZ_SCAN_CTL_WORDS, 0), frame_order, scan_wave;
    if (arena) {
        blk_desc.resize(a.chain_capacity / (4 + CZ_CHAIN_MAP_WORDS + 1) + 4096);
        a.blk_desc = blk_desc.data(); a.blk_capacity = (uint32_t)blk_desc.size(); a.scan_ctl = scan_ctl.data();
        frame_order.resize(n ? n : 1); a.frame_order = frame_order.data();
        scan_wave.assign(((n + 63) / 64 + 1) * 72, 0); a.scan_wave = scan_wave.data();
    }
    a.chain_grid = (uint32_t)grid;
    /* launches as the host library orders them with a dictionary setting (no execute stage) */
    const int order[7] = {4, 5, 0, 9, 7, 8, 1};
    for (int pi = 0; pi < 7; pi++) {
        const int which = order[pi];
        if (!arena && which != 1) continue;
        if ((which == 7 || which == 8 || which == 9) && !lit_bytes) continue;
        const int nthreads = which == 7 ? CZH_THREADS : (which == 8 ? 256 : 64);
        const int nblocks = which == 4 || which == 5 ? (int)((n + 63) / 64) : (which == 7 || which == 8 || which == 9 ? 1 : grid);
        cz_batch_args k = a;
        if (which == 4 || which == 5) k.scan_pass = (uint32_t)(which - 4);   /* 4, 5: the two passes of the block scan */
        emu_launch(nblocks, nthreads, [&] {
            if (which == 0) cz_chain_kernel(k);
            else if (which == 7) cz_huf_kernel(k);
            else if (which == 9) cz_huf1_kernel(k);
            else if (which == 8) cz_tile_kernel(k);
            else if (which >= 4) cz_scan_kernel(k);
            else cz_decode_frames_kernel(k);
        });
    }
    if (lit_bytes) {
        unsigned long long nd = 0; for (uint64_t i = 0; i < n; i++) nd += (frame_pre[i] & CZ_PRE_DONE) != 0;
        fprintf(stderr, "EMU_LIT: %llu frames finished by the pre-pass\n", nd);
    }
    const int dump_all = getenv("EMU_DUMP_ALL") && atoi(getenv("EMU_DUMP_ALL")) > 0;
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    for (uint64_t i = 0; i < n; i++) {
        fwrite(&res[i], sizeof(cz_frame_result), 1, g);
        const uint64_t w = dump_all ? out_cap[i] : (res[i].bytes_produced <= out_cap[i] ? res[i].bytes_produced : out_cap[i]);
        fwrite(out + out_off[i], 1, w, g);
    }
    fclose(g);
    free(in_exact); free(out); free(lit); free(arena); free(lit_arena); free(dicts);
    return 0;
}
