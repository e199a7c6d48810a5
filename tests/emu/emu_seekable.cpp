/*
 * TEST INFRASTRUCTURE ONLY — runs the seekable-stream kernels (cz_seekable_plan_kernel, cz_seekable_gather_kernel and
 * cz_seekable_open_kernel; the unmodified czstd_seekable.hip behind czstd_kernels.hip) on the CPU through tests/emu/hip/hip_runtime.h,
 * under ASan+UBSan: one workgroup of 256 lanes at a time, a grid of three for the gather, so that a workgroup takes tiles a stride
 * apart.  Workgroups run one after another, which is all these kernels need: none waits for another.
 * usage: emu_seekable <cases.bin> <result.bin>        (both as seekable_cases.h says; the return value written is always 0)
 * result.bin starts with u64 the gather's tile in bytes.  Every frame, the records, the offsets, the plan (n + 2 words, 0xA5 before
 * the plan kernel), the stream and the arrays are heap blocks of their exact size.
 */
#define EMU_ENCODE
#include "emu_harness.h"
#include "czstd_seekable.hip"
#include "seekable_cases.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    FILE* g = fopen(argv[2], "wb"); if (!g) return 2;
    { const uint64_t tile = 16ull * CZS_TILE_VECS; fwrite(&tile, 8, 1, g); }
    for (int kind; (kind = fgetc(f)) != EOF;) {
        cz_seekable_info* info = (cz_seekable_info*)malloc(sizeof(cz_seekable_info)); memset(info, 0xA5, sizeof *info);
        if (kind == 'P') {
            sk_pack_case c; if (!sk_read_pack(f, &c)) return 2;
            unsigned long long* plan = (unsigned long long*)malloc((c.n + 2) * sizeof(unsigned long long));
            memset(plan, 0xA5, (c.n + 2) * sizeof(unsigned long long));
            emu_launch(1, CZS_THREADS, [&] { cz_seekable_plan_kernel(c.d_res, (uint32_t)c.n, c.flags, c.cap, plan, info); });
            cz_seekable_gather_args a; memset(&a, 0, sizeof a);
            a.frames_base = c.base; a.frame_off = c.d_off; a.results = c.d_res; a.plan = plan; a.stream = c.stream; a.n = (uint32_t)c.n; a.flags = c.flags;
            emu_launch(3, CZS_THREADS, [&] { cz_seekable_gather_kernel(a); });
            sk_write_pack(g, &c, 0, info);
            free(plan);
        } else if (kind == 'O') {
            sk_open_case c; if (!sk_read_open(f, &c)) return 2;
            cz_seekable_open_args a; memset(&a, 0, sizeof a);
            a.stream = c.stream; a.stream_len = c.len; a.first = c.first; a.count = c.count; a.out_align = c.align; a.info = info;
            if (c.arrays) { a.in_off = c.a[0]; a.in_len = c.a[1]; a.out_off = c.a[2]; a.out_cap = c.a[3]; a.checksum = c.sums; }
            emu_launch(1, CZS_THREADS, [&] { cz_seekable_open_kernel(a); });
            sk_write_open(g, &c, 0, info);
        } else return 2;
        free(info);
    }
    fclose(f); fclose(g);
    return 0;
}
