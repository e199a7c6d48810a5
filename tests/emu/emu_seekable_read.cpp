/*
 * TEST INFRASTRUCTURE ONLY — runs the seekable-read kernels (cz_seekable_index_kernel, cz_seekable_locate_kernel,
 * cz_seekable_select_kernel and cz_seekable_ranges_kernel; the unmodified czstd_seekable_read.hip behind czstd_seekable.hip) on the
 * CPU through tests/emu/hip/hip_runtime.h, under ASan+UBSan, launched in the order of the library's host functions: the open
 * kernel on no frames and the index kernel (one workgroup each), then per locate the range kernel on as many workgroups of 256 as
 * the ranges need and the selection kernel on one, and a grid of three for the gather, so that a workgroup takes tiles a stride
 * apart.  Workgroups run one after another, which is all these kernels need: none waits for another.
 * usage: emu_seekable_read <cases.bin> <result.bin>   (both as seekable_read_cases.h says; a locate's return value is its info's status)
 * result.bin starts with u64 the gather's tile in bytes.  The index's arrays (comp and cont of n + 1, sums, reach and sel_off of n
 * entries), rng (2 m words per call), the bad-range word and every array of the case are heap blocks of their exact size.
 */
#define EMU_ENCODE
#include "emu_harness.h"
#include "czstd_seekable.hip"
#include "czstd_seekable_read.hip"
#include "seekable_read_cases.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    { const uint64_t tile = 16ull * CZS_TILE_VECS; fwrite(&tile, 8, 1, g); }
    for (int kind; (kind = fgetc(f)) != EOF;) {
        if (kind == 'L') {
            sr_stream s; if (!sr_read_stream(f, &s)) return 2;
            cz_seekable_info* table = sr_block<cz_seekable_info>(1, 0xA5);
            cz_seekable_open_args o; memset(&o, 0, sizeof o);
            o.stream = s.bytes; o.stream_len = s.len; o.first = 0; o.count = 0; o.out_align = 1; o.info = table;
            emu_launch(1, CZS_THREADS, [&] { cz_seekable_open_kernel(o); });
            const int st = table->status;
            fwrite(&st, 4, 1, g); fwrite(table, sizeof *table, 1, g);
            if (st != CZ_OK) { if (s.calls) return 2; free(table); free(s.bytes); continue; }
            const uint64_t n = table->frames;
            unsigned long long* comp = sr_block<unsigned long long>(n + 1, 0xA5); unsigned long long* cont = sr_block<unsigned long long>(n + 1, 0xA5);
            unsigned long long* sel_off = sr_block<unsigned long long>(n, 0xA5);
            uint32_t* sums = sr_block<uint32_t>(n, 0xA5); uint32_t* reach = sr_block<uint32_t>(n, 0xA5); uint32_t* bad = sr_block<uint32_t>(1, 0);
            cz_seekable_index_args ia; memset(&ia, 0, sizeof ia);
            ia.stream = s.bytes; ia.stream_len = s.len; ia.n = n; ia.E = table->has_checksums ? 12u : 8u;
            ia.comp = comp; ia.cont = cont; ia.sums = sums; ia.reach = reach;
            emu_launch(1, CZS_THREADS, [&] { cz_seekable_index_kernel(ia); });
            free(s.bytes); s.bytes = nullptr;                           /* the stream need not outlive the index */
            for (uint32_t q = 0; q < s.calls; q++) {
                sr_call c; if (!sr_read_call(f, &c)) return 2;
                cz_seekable_read_info* info = sr_block<cz_seekable_read_info>(1, 0xA5);
                uint32_t* rng = sr_block<uint32_t>(2 * c.m, 0xA5);
                if (c.m) {
                    cz_seekable_locate_args a; memset(&a, 0, sizeof a);
                    a.cont = cont; a.n = n; a.range_off = c.off; a.range_len = c.len; a.m = c.m; a.reach = reach; a.rng = rng; a.bad = bad;
                    emu_launch((int)((c.m + CZS_THREADS - 1) / CZS_THREADS), CZS_THREADS, [&] { cz_seekable_locate_kernel(a); });
                }
                cz_seekable_select_args a; memset(&a, 0, sizeof a);
                a.comp = comp; a.cont = cont; a.sums = sums; a.reach = reach; a.sel_off = sel_off; a.rng = rng; a.bad = bad;
                a.n = n; a.has_checksums = table->has_checksums; a.out_align = c.align; a.frames_cap = c.frames_cap;
                a.range_off = c.off; a.range_len = c.len; a.m = c.m; a.info = info;
                if (c.arrays) {
                    a.frame = c.frame; a.in_off = c.a[0]; a.in_len = c.a[1]; a.out_off = c.a[2]; a.out_cap = c.a[3]; a.checksum = c.sums;
                    a.content_off = c.content_off; a.spans = c.spans;
                }
                emu_launch(1, CZS_THREADS, [&] { cz_seekable_select_kernel(a); });
                uint8_t clean = *bad == 0;
                for (uint64_t i = 0; i < n; i++) if (reach[i]) clean = 0;
                sr_write_call(g, &c, info->status, info, clean);
                free(rng); free(info);
            }
            free(comp); free(cont); free(sel_off); free(sums); free(reach); free(bad); free(table);
        } else if (kind == 'G') {
            sr_gather_case c; if (!sr_read_gather(f, &c)) return 2;
            if (c.m && c.dst_bytes) {                                   /* (the host function launches nothing otherwise) */
                cz_seekable_ranges_args a; memset(&a, 0, sizeof a);
                a.decoded = c.decoded; a.out_off = (const unsigned long long*)c.out_off; a.content_off = (const unsigned long long*)c.content_off;
                a.range_off = c.off; a.range_len = c.len; a.spans = c.spans; a.m = (uint32_t)c.m; a.dst = c.dst; a.dst_bytes = c.dst_bytes;
                emu_launch(3, CZS_THREADS, [&] { cz_seekable_ranges_kernel(a); });
            }
            sr_write_gather(g, &c, 0);
        } else return 2;
    }
    fclose(f); fclose(g);
    return 0;
}
