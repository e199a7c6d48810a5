/* czstd_dict.h — the table of dictionaries a batch picks from by Dictionary_ID (cz_context_set_dictionaries), shared by the
 * host side, cz_scan_kernel (czstd_chain.hip), cz_decode_frames_kernel (czstd_kernels.hip) and the CPU emulator of tests/emu. */
#ifndef CZSTD_DICT_H
#define CZSTD_DICT_H

#include <stdint.h>

/* One registered dictionary, in HBM; the table is sorted by id (ascending, no duplicates, no 0). */
typedef struct cz_dict_entry {
    uint32_t id; uint32_t pad;
    const struct cz_device_frame_state* state;   /* tables and repeat offsets as cz_dict_setup_kernel left them */
    const uint8_t* content; uint64_t content_len;  /* DecodeBuffer.dict_content */
} cz_dict_entry;

/* What a frame whose header names no ID (or ID 0) gets: the no_id dictionary of the batch; what one that names an ID not in the
   table gets: nothing, and the frame fails with CZ_E_DICT_UNKNOWN */
#define CZ_DICT_NO_ID  0xFFFFFFFFu
#define CZ_DICT_UNKNOWN 0xFFFFFFFEu

/* index of `id` in the table, CZ_DICT_NO_ID for id 0, CZ_DICT_UNKNOWN when it is not there (binary search: at most 11 steps for
   the 1024 entries the host allows) */
__host__ __device__ static inline uint32_t cz_dict_find(const cz_dict_entry* t, uint32_t k, uint32_t id) {
    if (id == 0) return CZ_DICT_NO_ID;
    uint32_t lo = 0, hi = k;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1, v = t[mid].id;
        if (v == id) return mid;
        if (v < id) lo = mid + 1; else hi = mid;
    }
    return CZ_DICT_UNKNOWN;
}

/* Dictionary_ID of a frame header (frame.cairo:207-225) whose bytes are at p and that has been found complete (the whole header is there):
   0 when it has no ID field.  The field begins behind the descriptor and, in a frame that is not single-segment, the window byte. */
template <typename P> __host__ __device__ static inline uint32_t cz_frame_dict_id(P p) {   /* P: a pointer to the frame's bytes, in whichever address space */
    const uint32_t d = p[4], didf = d & 3, at = 5 + (((d >> 5) & 1) ? 0 : 1);
    if (!didf) return 0;
    uint32_t id = p[at];
    if (didf >= 2) id |= (uint32_t)p[at + 1] << 8;
    if (didf == 3) id |= ((uint32_t)p[at + 2] << 16) | ((uint32_t)p[at + 3] << 24);
    return id;
}

#endif
