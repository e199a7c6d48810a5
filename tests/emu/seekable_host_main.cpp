/*
 * TEST INFRASTRUCTURE ONLY — cz_seekable_pack_host and cz_seekable_open_host (csrc/czstd_seekable_host.h, plain C++) in a
 * stand-alone program under ASan+UBSan: no HIP, no library, no preloading.  Reads the cases of seekable_cases.h, runs each on
 * exact-size heap blocks and writes what came out.
 * usage: seekable_host_main <cases.bin> <result.bin>
 */
#include "seekable_cases.h"
#include "czstd_seekable_host.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    for (int kind; (kind = fgetc(f)) != EOF;) {
        cz_seekable_info info; memset(&info, 0xA5, sizeof info);
        if (kind == 'P') {
            sk_pack_case c; if (!sk_read_pack(f, &c)) return 2;
            const int ret = cz_seekable_pack_host(c.base, c.d_off, c.d_res, (size_t)c.n, c.stream, c.cap, c.flags, &info);
            sk_write_pack(g, &c, ret, &info);
        } else if (kind == 'O') {
            sk_open_case c; if (!sk_read_open(f, &c)) return 2;
            const int ret = c.arrays ? cz_seekable_open_host(c.stream, c.len, c.first, c.count, c.align, c.a[0], c.a[1], c.a[2], c.a[3], c.sums, &info)
                                     : cz_seekable_open_host(c.stream, c.len, c.first, c.count, c.align, nullptr, nullptr, nullptr, nullptr, nullptr, &info);
            sk_write_open(g, &c, ret, &info);
        } else return 2;
    }
    fclose(f); fclose(g);
    return 0;
}
