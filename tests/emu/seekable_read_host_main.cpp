/*
 * TEST INFRASTRUCTURE ONLY — cz_seekable_locate_host and cz_seekable_gather_host (csrc/czstd_seekable_read_host.h, plain C++) in a
 * stand-alone program under ASan+UBSan: no HIP, no library, no preloading.  Reads the cases of seekable_read_cases.h, runs each on
 * exact-size heap blocks and writes what came out.  The "index" of an 'L' case is cz_seekable_open_host of no frames.
 * usage: seekable_read_host_main <cases.bin> <result.bin>
 */
#include "seekable_read_cases.h"
#include "czstd_seekable_read_host.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    for (int kind; (kind = fgetc(f)) != EOF;) {
        if (kind == 'L') {
            sr_stream s; if (!sr_read_stream(f, &s)) return 2;
            cz_seekable_info table; memset(&table, 0xA5, sizeof table);
            const int st = cz_seekable_open_host(s.bytes, s.len, 0, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, &table);
            fwrite(&st, 4, 1, g); fwrite(&table, sizeof table, 1, g);
            for (uint32_t q = 0; q < s.calls; q++) {
                sr_call c; if (!sr_read_call(f, &c)) return 2;
                cz_seekable_read_info info; memset(&info, 0xA5, sizeof info);
                const int ret = c.arrays ? cz_seekable_locate_host(s.bytes, s.len, c.off, c.len, (size_t)c.m, c.align, c.frames_cap, c.frame, c.a[0], c.a[1], c.a[2],
                                                                   c.a[3], c.sums, c.content_off, c.spans, &info)
                                         : cz_seekable_locate_host(s.bytes, s.len, c.off, c.len, (size_t)c.m, c.align, c.frames_cap, nullptr, nullptr, nullptr,
                                                                   nullptr, nullptr, nullptr, nullptr, nullptr, &info);
                if (st == CZ_OK) sr_write_call(g, &c, ret, &info, 1);
            }
            free(s.bytes);
        } else if (kind == 'G') {
            sr_gather_case c; if (!sr_read_gather(f, &c)) return 2;
            const int ret = cz_seekable_gather_host(c.decoded, c.out_off, c.content_off, c.k, c.off, c.len, c.spans, (size_t)c.m, c.dst, c.dst_bytes);
            sr_write_gather(g, &c, ret);
        } else return 2;
    }
    fclose(f); fclose(g);
    return 0;
}
