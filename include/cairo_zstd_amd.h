/*
 * cairo_zstd_amd.h — C ABI of the MI355X-native zstd decoder (libcairo_zstd_amd.so).
 *
 * The reference (NethermindEth/cairo_zstd, pure Cairo 1) has no FFI of its own
 * (SURVEY.md §8b); the boundary is therefore its *trait API*, re-exposed here as plain C:
 * opaque handles, plain pointers and sizes, int32 status codes that map 1:1 onto the
 * reference's error-enum leaves (cairo_zstd_amd_status.h).  Every entry point cites the
 * reference interface it replaces (file:line relative to the reference tree).
 * INTEGRATION.md shows the Cairo-runner-hint / ctypes binding a maintainer would add.
 *
 * Three layers:
 *   1. cz_context_*        device context (HIP stream, scratch arenas).     [no reference analogue]
 *   2. cz_decode_batch*    many independent frames in one launch — the GPU hot path.
 *                          Semantics per frame = `_test_decode` (src/tests/decoding.cairo:4-21).
 *   3. cz_frame_decoder_*  one resumable frame, mirrors FrameDecoderTrait
 *                          (src/frame_decoder.cairo:107-335) call for call.
 *   plus stateless header parsers mirroring read_frame_header / read_block_header.
 *
 * Threading: one context / frame decoder per host thread.  Batch calls are asynchronous on
 * the context's HIP stream unless stated otherwise.  All compute runs on the device; there
 * is no CPU decode path in this library — without a gfx950 device every compute entry
 * returns CZ_E_NO_DEVICE.
 */
#ifndef CAIRO_ZSTD_AMD_H
#define CAIRO_ZSTD_AMD_H

#include <stddef.h>
#include <stdint.h>

#include "cairo_zstd_amd_status.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CZ_ABI_VERSION 1

/* Per-frame result record written by the device (one per batch entry).  Mirrors what the
 * reference exposes after decode_blocks: is_finished (frame_decoder.cairo:144),
 * blocks_decoded (:152), bytes_read_from_source (:140), get_checksum_from_data (:129). */
typedef struct cz_frame_result {
    int32_t  status;            /* cz_status */
    uint32_t blocks_decoded;
    uint64_t bytes_consumed;    /* source bytes consumed, frame header and checksum included */
    uint64_t bytes_produced;    /* decoded bytes written at out_base + out_off[i] */
    uint32_t checksum_from_data;/* valid when flags & CZ_RESULT_HAS_CHECKSUM */
    uint32_t flags;
    uint64_t detail[2];         /* error payload (e.g. magic / skip length for CZ_E_FH_SKIP_FRAME,
                                   block index and byte position for decode errors) */
    uint32_t calculated_checksum; /* low 32 bits of XXH64(decoded frame), valid when flags & CZ_RESULT_CHECKSUM_COMPUTED
                                   (get_calculated_checksum, frame_decoder.cairo:133-138) */
    uint32_t reserved;
} cz_frame_result;
#define CZ_RESULT_FINISHED     1u   /* last block seen (frame_finished, frame_decoder.cairo:190) */
#define CZ_RESULT_HAS_CHECKSUM 2u
#define CZ_RESULT_CHECKSUM_COMPUTED 4u  /* cz_context_set_verify_checksum(ctx, 1): XXH64 was computed on the device */
#define CZ_RESULT_CHECKSUM_MATCH    8u  /* ... and equals checksum_from_data */

/* ---------------------------------------------------------------- 1. context */
typedef struct cz_context cz_context;

int  cz_abi_version(void);
/* Creates a decoder context on HIP device `device` (ordinal).  `stream` may be NULL (the
 * context then owns a NON-BLOCKING stream) or a hipStream_t cast to void*.  NULL is also the handle of the legacy default
 * stream: a caller whose other work runs there (PyTorch's torch.cuda.current_stream().cuda_stream is 0 unless a stream
 * context is active) gets a context that is NOT ordered with that work — it must synchronise (or record / wait on events)
 * between filling the buffers a batch call reads or writes and the call, and again before it reads the results, or pass a
 * stream of its own making. */
int  cz_context_create(cz_context** out, int device, void* stream);
void cz_context_destroy(cz_context* ctx);
int  cz_context_synchronize(cz_context* ctx);
/* Last HIP error seen by this context (hipError_t), for CZ_E_HIP diagnostics. */
int  cz_context_last_hip_error(const cz_context* ctx);
/* Kernel-launch geometry actually used (for bench / roofline reports). */
int  cz_context_launch_info(const cz_context* ctx, int* workgroups, int* threads_per_wg, int* compute_units);
/* Waves the execute-stage kernels of a batch launch run with: cz_execute_frames_kernel (4 waves per SIMD) and its 8-waves build. */
int  cz_context_execute_grid(const cz_context* ctx, int* waves, int* waves8);

/* ------------------------------------------------------- 2. batch (GPU hot path) */
/*
 * Decodes n independent zstd frames.  Frame i occupies in_base[in_off[i] .. +in_len[i]) and is
 * decoded to out_base[out_off[i] .. +out_cap[i]).  Each frame is handled exactly like the
 * reference's end-to-end entry: FrameDecoderStateTrait::new (frame_decoder.cairo:54) ->
 * decode_blocks(All) (:156) -> is_finished (:144); results[i] carries what the getters return.
 * A frame that fails leaves its neighbours untouched.
 *
 * ALL pointers are DEVICE pointers (results too).  Asynchronous on the context stream.
 * Returns CZ_OK when the launch was enqueued; per-frame outcomes are in results[].
 */
int cz_decode_batch_device(cz_context* ctx,
                           const void* d_in_base, const uint64_t* d_in_off, const uint64_t* d_in_len, size_t n,
                           void* d_out_base, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                           cz_frame_result* d_results);

/* Same, with HOST buffers: stages the inputs to the device, decodes, copies outputs and
 * results back, and synchronizes.  (PCIe-inclusive convenience path.) */
int cz_decode_batch_host(cz_context* ctx,
                         const void* in_base, size_t in_bytes, const uint64_t* in_off, const uint64_t* in_len, size_t n,
                         void* out_base, size_t out_bytes, const uint64_t* out_off, const uint64_t* out_cap,
                         cz_frame_result* results);

/* Several devices: frames share nothing (FrameDecoderStateTrait::reset, src/frame_decoder.cairo:78-104),
 * so a batch shards by frame with no exchange between the devices.
 *
 * cz_partition_balanced deals n items of the given weights (a frame's algorithmic bytes: compressed + decoded) to `parts`
 * parts so that the sums are balanced — heaviest first, each to the part that is lightest so far, ties to the lower index:
 * deterministic, every caller computes the same dealing.  part_of[i] = part of item i.  No device needed.
 *
 * cz_decode_batch_multi decodes ONE batch of host buffers on n_ctx contexts (normally one per GPU of the node): it deals the
 * frames with cz_partition_balanced (weight = in_len + out_cap), runs every share through cz_decode_batch_host on a thread
 * of its own — stage, launch, copy back, all concurrently across the devices — and leaves outputs and results in the
 * caller's layout, exactly as one cz_decode_batch_host call would.  device_of (optional, n entries): the context index every
 * frame went to.  Every context keeps its own arenas and options (cz_context_set_chain_arena ... per context); a context may
 * appear once.  A share is packed once, into pinned staging memory the context keeps. */
int cz_partition_balanced(const uint64_t* weights, size_t n, size_t parts, uint32_t* part_of);
/* ... and without host buffers (no PCIe in the path): the caller has dealt the frames (cz_partition_balanced) and put every share
 * on its device; cz_decode_batch_multi_device launches share d on context d (cz_decode_batch_device: it only enqueues, so the
 * devices run concurrently).  A context may appear once.
 * cz_gather_to_root is the one exchange the path has: `bytes[d]` bytes at d_src[d] on context d's device go
 * to d_dst_on_root[d] on the root context's device, every d != root — n_ctx - 1 concurrent peer copies (hipMemcpyPeerAsync), each on
 * its source context's stream behind that context's decode, so that all of the root's xGMI links carry traffic; the root's stream
 * waits for them.  Entry `root` of the three arrays is ignored. */
typedef struct cz_device_share {
    const void* d_in_base; const uint64_t* d_in_off; const uint64_t* d_in_len; size_t n;
    void* d_out_base; const uint64_t* d_out_off; const uint64_t* d_out_cap; cz_frame_result* d_results;
} cz_device_share;
int cz_decode_batch_multi_device(cz_context* const* ctxs, size_t n_ctx, const cz_device_share* shares);
int cz_gather_to_root(cz_context* const* ctxs, size_t n_ctx, size_t root, const void* const* d_src, const size_t* bytes, void* const* d_dst_on_root);
int cz_decode_batch_multi(cz_context* const* ctxs, size_t n_ctx,
                          const void* in_base, size_t in_bytes, const uint64_t* in_off, const uint64_t* in_len, size_t n,
                          void* out_base, size_t out_bytes, const uint64_t* out_off, const uint64_t* out_cap,
                          cz_frame_result* results, uint32_t* device_of);

/* Enables (bytes > 0) or disables (0) the FSE-chain pre-pass for batch decodes on this context and sizes its record
 * arena (8 bytes per sequence + 1312 per block with sequences; 8x the compressed bytes + 64 MiB covers every BASELINE
 * config).  With the pre-pass a batch decode is: cz_scan_kernel twice (lists the blocks of all frames, sorted by
 * sequence count, and allocates their arena space) -> cz_chain_kernel (ten blocks per wave, the three FSE state
 * machines of a block on three lanes; writes one record per sequence) -> the frame kernels, which consume the
 * records (sequence_section_decoder.cairo:223-297 is what the records replace).  Frames the arena cannot hold, or
 * that are irregular in any way, are decoded entirely by cz_decode_frames_kernel: errors are only ever reported by it. */
int cz_context_set_chain_arena(cz_context* ctx, size_t bytes);
/* Enables (bytes > 0) or disables (0) the rest of the pre-pass, which needs the chain arena too: cz_scan_kernel also lists
 * every Huffman-coded literals section and every run of bytes whose place in the output is known without decoding
 * (Raw / RLE blocks ahead of a frame's first block with sequences); the sections are decoded block-parallel
 * (tree description, table, streams: literals_section_decoder.cairo:58-243) by cz_huf1_kernel NEXT TO cz_chain_kernel and
 * cz_huf_kernel behind it — into nodes of an arena of `bytes` (decoded literal bytes + 16 per block; at most the decoded
 * size of the batch), or straight into the output for blocks without sequences — and the runs are copied by
 * cz_tile_kernel.  Frames the pre-pass finishes need no frame kernel at all; the others go to cz_execute_frames_kernel
 * (sequence execution only: sequence_execution.cairo:12-129) unless cz_context_set_exec_kernel turned it off; frames that
 * did not fit, or that are irregular in any way, are decoded from scratch by cz_decode_frames_kernel in the same call. */
int cz_context_set_literal_arena(cz_context* ctx, size_t bytes);
/* What the two arenas must hold for a batch that already sits on the device, from its headers alone (cz_scan_kernel's counting pass:
 * block_decoder.cairo:237-321, literals_section.cairo:81-175, sequence_section.cairo:77-114; nothing is decoded): 8 bytes per
 * sequence + 1 312 per block with sequences, and the Huffman-coded literals of blocks with sequences + 16 per block.  For set-up
 * (it synchronises): size the arenas once for the largest batch a caller will decode — a rule of thumb (8 x the compressed bytes)
 * takes 2.5 x as much for config 4a. */
int cz_context_measure_batch(cz_context* ctx, const void* d_in_base, const uint64_t* d_in_off, const uint64_t* d_in_len, size_t n,
                             const uint64_t* d_out_cap, size_t* chain_arena_bytes, size_t* literal_arena_bytes);
/* Frames whose first sequences section holds fewer sequences than `n` skip the pre-pass (default 0: every frame
 * with sequences takes it — the pre-pass works block by block, so short chains cost little). */
int cz_context_set_chain_min_sequences(cz_context* ctx, uint32_t n);

/* Batch decodes also compute the XXH64 content checksum of every frame that carries one, on the
 * device, and compare it with the stored value (what `_test_decode` asserts,
 * src/tests/decoding.cairo:16-19).  A mismatch is reported in the result flags, not as a status:
 * the reference leaves the comparison to the caller too.  Off by default. */
int cz_context_set_verify_checksum(cz_context* ctx, int on);

/* Duration in milliseconds of the most recent decode launch on this context, measured with
 * hipEvents recorded on the context stream around the kernel (bench.py's roofline leg).
 * Blocks until that launch has finished. */
int cz_context_last_kernel_ms(cz_context* ctx, float* ms);
/* The part of it spent in the FSE-chain pre-pass kernel (0 when the pre-pass is off). */
int cz_context_last_chain_ms(cz_context* ctx, float* ms);
/* Diagnostics of the most recent batch launch of n frames (synchronises): frames that got chain records from the
 * pre-pass, frames whose literals the huff0 kernels decoded. */
int cz_context_last_prepass_counts(cz_context* ctx, size_t n, size_t* with_chain, size_t* with_literals);
/* How long that launch went on with cz_huf_kernel / cz_huf1_kernel / cz_tile_kernel after the chain kernel was done
 * (0: no literal arena). */
int cz_context_last_literals_tail_ms(cz_context* ctx, float* ms);
/* The part of it spent in cz_execute_frames_kernel (0 when it did not run). */
int cz_context_last_exec_ms(cz_context* ctx, float* ms);
/* With both arenas set, frames the pre-pass prepared completely are executed by cz_execute_frames_kernel (one wave per
 * frame, sequence execution only: no decoders in LDS or registers) — on = 1, the default; on = 0 sends them to
 * cz_decode_frames_kernel's record path instead (the round-2 arrangement, kept for A/B runs: bench.py --no-exec-kernel).
 * Batches that start from a dictionary (cz_context_set_dictionary / cz_context_set_dictionaries) always take cz_decode_frames_kernel. */
int cz_context_set_exec_kernel(cz_context* ctx, int on);   /* (on = 4 / 8: that register budget — waves per SIMD — whatever the batch looks like; 1: decided on the device) */
/* With both arenas set, the frames that hold enough sequences to be worth a workgroup can also be executed by cz_wexec_kernel:
 * 16 waves per frame, the output of the block in hand in a 128 KiB LDS window (earlier blocks are read from the output buffer;
 * a block that regenerates more than the window is done in several passes), the three values the reference carries from sequence
 * to sequence (output position, literal cursor, offset history: sequence_execution.cairo:12-129, scratch.cairo:11-19) composed
 * across chunks of 64 sequences by a look-back, match sources ordered byte by byte through a bitmap of final bytes.  It runs SIDE BY
 * SIDE with cz_execute_frames_kernel, on half of the CUs, and the two share the frames (each claims a frame before it starts on
 * it): one is bound by instruction issue, the other by the rate of random reads from HBM.  Whether a batch is executed this way is
 * decided on the device, from the offset-code tables of its blocks (cz_chain_kernel sums them up): only when far offsets outweigh
 * near ones — with near offsets the waves of a frame wait on each other's bytes and a workgroup is no faster than one wave.
 * A frame cz_wexec_kernel cannot finish (a check of execute_sequences fails) goes to cz_decode_frames_kernel, which reports the
 * reference's status.  on = 1, the default; on = 0: cz_execute_frames_kernel alone (A/B runs: bench.py --no-wexec-kernel). */
int cz_context_set_wexec_kernel(cz_context* ctx, int on);
/* A/B knobs: CUs cz_wexec_kernel runs on (0: half of them), frames per such CU that cz_execute_frames_kernel leaves to it at the end
 * of a batch (0: the default, 7), force = 1: side by side whatever the batch's offsets look like (tests use it); force = 2: never
 * cz_wexec_kernel on a near-offset batch (by default it takes such a batch's few large frames — 36 000 sequences and more — when
 * the batch has 2 048 frames or more: each has a CU to itself there instead of a wave among 4 096). */
int cz_context_set_wexec_tuning(cz_context* ctx, int cus, int leave_per_cu, int force);
/* Diagnostics of the most recent batch launch (synchronises): what cz_chain_kernel summed from the blocks' LL / OF / ML code
 * tables, in sequences x 4 — with near offset codes (2..13: offsets below 16 KiB), with far ones, with a literal run above 8 or a
 * match above 16 bytes.  The execute stage is arranged from these on the device: cz_wexec_kernel beside cz_execute_frames_kernel
 * when far > near; the 8-waves-per-SIMD build of cz_execute_frames_kernel when near > far and long < (near + far) / 256. */
int cz_context_last_sequence_stats(cz_context* ctx, uint64_t* near_offsets, uint64_t* far_offsets, uint64_t* long_runs);
/* Diagnostics of the most recent batch launch (synchronises): frames listed for cz_wexec_kernel, frames it finished, frames it
 * handed on to cz_decode_frames_kernel. */
int cz_context_last_wexec_counts(cz_context* ctx, size_t* listed, size_t* finished, size_t* given_up);
/* Diagnostics of the most recent batch launch (synchronises), side by side: workgroups of cz_wexec_kernel that counted themselves in,
 * waves of cz_execute_frames_kernel that left the CUs to it (never every wave of a launch), waves that waited for it and stayed. */
int cz_context_last_side_counts(cz_context* ctx, size_t* wexec_in, size_t* exec_left, size_t* exec_waited);
/* The chain pre-pass of a batch is two launches of cz_chain_kernel — the LARGE blocks (4 096 sequences and more: a batch lasts as
 * long as its longest chain, sequence_section_decoder.cairo:223-286) on one stream, all others on another — and the execute stage
 * starts behind the second: cz_execute_frames_kernel on every frame without a large block, cz_wexec_kernel on the batch's large
 * frames, block by block behind their chains (frames share nothing: src/frame_decoder.cairo:78-104).  on = 0: one chain launch,
 * the execute stage behind all of it.  Default 0: measured in round 5, the arrangement does not pay yet (profiles/r5/NOTES.md): kept
 * as an experiment, covered by the GPU suite. */
int cz_context_set_early_execute(cz_context* ctx, int on);
/* When the small blocks' chains and every literal of the most recent launch were done, in ms from its start (0: not such a launch). */
int cz_context_last_small_ms(cz_context* ctx, float* ms);
/* Diagnostics of the most recent batch launch (synchronises): entries on the fall-back list — frames the pre-pass and execute
 * kernels handed to cz_decode_frames_kernel, each listed once whoever handed it back.  The list has no analogue in the reference:
 * it is the device-side form of "decode this frame by the reference's own order of steps" (src/frame_decoder.cairo:156-222). */
int cz_context_last_fallback_count(cz_context* ctx, size_t* listed);
/* A batch decode enqueues about 35 stream operations (kernels, events, joins).  When a launch repeats the one before it — the same
 * pointers, sizes and context settings; the bytes behind the pointers may differ — it is captured as a hipGraph, and from then on
 * such a launch is ONE graph submission (what a launch enqueues depends on its arguments and the context alone, never on the data).
 * on = 1 turns that on; default 0: every launch is enqueued operation by operation (measured: 3 % of a Raw/RLE batch, 7 % of a
 * batch of 2 000 frames, nothing on the entropy-coded configurations — profiles/r5/graph_replay_ab.txt).  Nothing in the reference
 * corresponds to this: it is how the loop "decode the next batch into the same buffers" (src/frame_decoder.cairo:156-222 called
 * frame after frame) can be submitted here.  A launch is only captured where cz_graph_replay_available() says so; elsewhere
 * every launch is enqueued operation by operation whatever `on` says. */
int cz_context_set_graph_replay(cz_context* ctx, int on);
/* 1 when launches can be captured in this process: the HIP runtime gives it more hardware queues (GPU_MAX_HW_QUEUES, 4 when
 * unset) than a capture has streams (3).  With fewer, the streams of a capture share queues, an arrangement in which capturing
 * crashed inside the ROCm 7.2 runtime. */
int cz_graph_replay_available(void);
/* 1 when the most recent batch launch was the replay of a captured graph. */
int cz_context_last_launch_was_replay(const cz_context* ctx);
/* The part of the most recent launch spent in cz_wexec_kernel (0 when it did not run). */
int cz_context_last_wexec_ms(cz_context* ctx, float* ms);

/* Test knobs (0 in normal use).  CZ_DEBUG_CHAIN_CPP_STEP: cz_chain_kernel takes every step of every chain with its plain C++ step
 * instead of the hand-scheduled inline-asm group — the two must leave the same records (sequence_section_decoder.cairo:223-286).
 * CZ_DEBUG_NO_HUF1: cz_huf1_kernel (the one-wave huff0 kernel beside the chain kernel) is not launched, so which kernel decodes a
 * literals section no longer depends on timing (literals_section_decoder.cairo:95-115: cz_huf_kernel hands a frame with an uneven
 * 4-stream split back, cz_huf1_kernel keeps it). */
#define CZ_DEBUG_CHAIN_CPP_STEP 1u
#define CZ_DEBUG_NO_HUF1 2u
#define CZ_DEBUG_WX_POISON 4u       /* cz_wexec_kernel: chunk 2 of every block never publishes its look-back entry, so every wave behind it waits until the
                                       bound of its polling loop (WX_SPIN_LIMIT) and the frame is handed to cz_decode_frames_kernel: the test of that bound */
#define CZ_DEBUG_EXEC_FIRST 8u      /* side by side: cz_execute_frames_kernel is submitted AHEAD of cz_wexec_kernel (normally behind it): the two keep to their halves
                                       of the CUs by the hardware's CU id, so the frames split the same way in either order — the test of that */
#define CZ_DEBUG_EXEC_LEAVE 16u     /* side by side: every wave of cz_execute_frames_kernel takes the leave branch at once, as if it were on an even CU that
                                       cz_wexec_kernel never met — the worst placement, made deterministic: the last wave stays and every frame is still decoded */
int cz_context_set_debug_flags(cz_context* ctx, uint32_t flags);
/* Copies the first `bytes` of the chain arena (headers, state -> code maps and per-sequence records of the most recent batch
 * launch, as cz_chain_kernel left them) to host memory and returns the arena units in use; synchronises.  For tests. */
int cz_context_debug_read_chain_arena(cz_context* ctx, void* dst, size_t bytes, uint64_t* units_in_use);

/* Diagnostic builds only (libcairo_zstd_amd_prof.so, -DCZ_PROFILE): copies out and clears the
 * per-phase shader-cycle sums accumulated by the kernels; returns the number of phases written
 * (0 in the product library, which executes no stamps). */
int cz_context_read_profile(cz_context* ctx, unsigned long long* out, int cap);

/* ------------------------------------------------- stateless header parsers */
/* read_frame_header (src/frame.cairo:152-284) + FrameHeaderTrait::window_size (:106-129). */
typedef struct cz_frame_header {
    uint8_t  descriptor;          /* FrameDescriptor (frame.cairo:25-27) */
    uint8_t  window_descriptor;
    uint8_t  has_dict_id;
    uint8_t  header_len;          /* bytes consumed */
    uint32_t dict_id;
    uint64_t frame_content_size;
    uint64_t window_size;
} cz_frame_header;
/* detail[0..1] = (magic, skip_len) for CZ_E_FH_SKIP_FRAME / CZ_E_FH_BAD_MAGIC; may be NULL. */
int cz_read_frame_header(const uint8_t* src, size_t len, cz_frame_header* out, uint64_t* detail);

/* BlockDecoderTrait::read_block_header (src/decoding/block_decoder.cairo:237-278);
 * BlockHeader (src/blocks/block.cairo:10-15).  Always consumes 3 bytes. */
typedef struct cz_block_header {
    uint8_t  last_block;
    uint8_t  block_type;          /* 0 Raw, 1 RLE, 2 Compressed (3 Reserved is an error) */
    uint32_t decompressed_size;   /* Raw/RLE: size; Compressed: 0 = unknown */
    uint32_t content_size;        /* Raw/Compressed: size; RLE: 1 */
} cz_block_header;
int cz_read_block_header(const uint8_t* src, size_t len, cz_block_header* out);

/* ------------------------------------------------- stream walker */
/* read_frame_header returns a skippable frame to its caller as the error SkipFrame(magic, length)
 * (src/frame.cairo:160-166); cz_stream_split is that caller for a stream of concatenated frames: it cuts the stream
 * into one entry per zstd frame (its end found by walking the block headers, no decoding) and steps over skippable
 * frames, so that a multi-frame .zst goes through cz_decode_batch_* in one launch. */
typedef struct cz_stream_entry {
    uint64_t offset, length;      /* bytes of the stream this entry covers */
    uint32_t kind;                /* CZ_STREAM_FRAME or CZ_STREAM_SKIPPABLE */
    uint32_t magic;               /* skippable frame: its magic number (0x184D2A50..5F) */
    uint64_t content_size;        /* zstd frame: frame_content_size of its header (0 when absent) */
    uint64_t out_bound;           /* zstd frame: Raw / RLE sizes + 128 KiB per compressed block: an output capacity that
                                     holds every frame the zstd format allows (the reference accepts larger blocks: D3) */
    uint64_t window_size;
} cz_stream_entry;
#define CZ_STREAM_FRAME 0u
#define CZ_STREAM_SKIPPABLE 1u
/* Fills entries[0 .. min(*count, cap)); *count = entries in the stream, *consumed = bytes they cover.  Returns CZ_OK
 * when the whole stream was cut up, CZ_E_TARGET_TOO_SMALL when cap < *count, or the status of the header that could
 * not be read (the entries before it are valid). */
int cz_stream_split(const uint8_t* src, size_t len, cz_stream_entry* entries, size_t cap, size_t* count, size_t* consumed);

/* ------------------------------------------------- block level (BlockDecoder + DecoderScratch) */
/* DecoderScratch (src/decoding/scratch.cairo:11-67): the state a frame carries from block to block — Huffman
 * table, three FSE tables + RLE symbols, offset history (1, 4, 8) — and its DecodeBuffer
 * (src/decoding/decode_buffer.cairo:9-15).  Both live in HBM; the handle is the `ref workspace: DecoderScratch` of
 * decode_block_content.  Only the last window_size bytes plus what was not drained yet stay resident. */
typedef struct cz_decoder_scratch cz_decoder_scratch;
int  cz_decoder_scratch_create(cz_context* ctx, uint64_t window_size, cz_decoder_scratch** out);   /* DecoderScratchTrait::new, scratch.cairo:23-40 */
int  cz_decoder_scratch_reset(cz_decoder_scratch* s, uint64_t window_size);                        /* reset, scratch.cairo:42-58 */
void cz_decoder_scratch_destroy(cz_decoder_scratch* s);
size_t cz_decoder_scratch_buffer_len(const cz_decoder_scratch* s);                                 /* buffer.len() */
uint64_t cz_decoder_scratch_total_output(const cz_decoder_scratch* s);                             /* bytes decoded into the buffer so far.  Equals buffer.total_output_counter except
                                                                                                      after matches copied WHOLLY from a dictionary: the reference's counter skips
                                                                                                      those (decode_buffer.cairo:85-90); the device keeps that lag for its window
                                                                                                      test but this getter does not subtract it */
/* DecodeBuffer::drain (decode_buffer.cairo:157-166): moves the whole buffer to dst and feeds the XXH64 state. */
int  cz_decoder_scratch_drain(cz_decoder_scratch* s, uint8_t* dst, size_t cap, size_t* written);
/* DecodeBuffer::drain_to_window_size (:145-155): 1 = Some (bytes beyond window_size moved), 0 = None, < 0 = -cz_status. */
int  cz_decoder_scratch_drain_to_window_size(cz_decoder_scratch* s, uint8_t* dst, size_t cap, size_t* written);
uint64_t cz_decoder_scratch_hash_digest(const cz_decoder_scratch* s);                              /* buffer.hash.digest(): XXH64 of what was drained */

/* ------------------------------------------------- dictionaries */
/* Dictionary (src/decoding/dictionary.cairo:11-18).  The reference parses dictionaries and can seed a DecoderScratch from one,
 * but none of its decoders ever does (frame_decoder.cairo never calls init_from_dict): the same two calls are offered here,
 * on the block level, and a workspace seeded from a dictionary decodes frames that were compressed with it — Repeat-mode /
 * Treeless first blocks use the dictionary's tables, repeat offsets start from its three, matches may reach into its content
 * (decode_buffer.cairo:65-93).  The parsed tables and the content live in HBM. */
typedef struct cz_dictionary cz_dictionary;
/* DictionaryTrait::decode_dict (dictionary.cairo:35-91).  Errors: CZ_E_DICT_BAD_MAGIC (detail[0] = the magic read),
 * CZ_E_DICT_TRUNCATED, or the HuffmanTableError / FSETableError leaf. */
int  cz_dictionary_decode(cz_context* ctx, const uint8_t* raw, size_t len, cz_dictionary** out, uint64_t* detail);
void cz_dictionary_destroy(cz_dictionary* d);
uint32_t cz_dictionary_id(const cz_dictionary* d);                                                 /* Dictionary.id */
size_t cz_dictionary_content_len(const cz_dictionary* d);                                          /* dict_content.len() */
int  cz_dictionary_offset_hist(const cz_dictionary* d, uint32_t out[3]);                           /* Dictionary.offset_hist */
/* DecoderScratchTrait::init_from_dict (scratch.cairo:60-65); call it on a fresh or reset workspace.  reset clears it again
 * (decode_buffer.cairo:38).  The dictionary must stay alive while the workspace uses it. */
int  cz_decoder_scratch_init_from_dict(cz_decoder_scratch* workspace, const cz_dictionary* d);
/* The batch form of the same call: every frame cz_decode_batch_* decodes on this context starts as init_from_dict leaves a
 * workspace (NULL: back to the default, no dictionary).  This is the many-small-records case dictionaries exist for; frames
 * whose first block leans on the dictionary's tables are decoded by cz_decode_frames_kernel alone (the pre-pass lists only
 * frames that define their own tables), the others take the pre-pass as usual.  The dictionary must outlive the launches. */
int  cz_context_set_dictionary(cz_context* ctx, const cz_dictionary* d);
/* Several dictionaries at once (libzstd's ZSTD_d_refMultipleDDicts): every later cz_decode_batch_* on this context (per context in
 * cz_decode_batch_multi*, and cz_decode_stream) picks each frame's dictionary by the Dictionary_ID of its header (frame.cairo:207-225):
 *   no ID field, or ID 0       -> no_id_dict, as init_from_dict leaves a workspace (NULL: no dictionary, a fresh workspace)
 *   cz_dictionary_id(dicts[j]) -> dicts[j]: its tables, its three repeat offsets, its content
 *   any other ID               -> CZ_E_DICT_UNKNOWN, detail[0] = the ID, bytes_produced = 0, the frame's output region untouched.
 * Header errors come first, as always (a truncated ID field is CZ_E_FH_DICT_ID_READ, a skippable frame CZ_E_FH_SKIP_FRAME);
 * CZ_E_DICT_UNKNOWN is reported after a complete header, before any block.  CZ_E_INVALID_ARG when dicts is NULL with k > 0, an entry
 * is NULL, a dictionary belongs to another context, a listed dictionary has ID 0 (it can only be no_id_dict), two listed ones share
 * an ID, or k > CZ_MAX_DICTIONARIES; on any error the previous setting stays in force.  k == 0 with no_id_dict NULL clears the
 * setting, like cz_context_set_dictionary(ctx, NULL); the two calls replace each other.  Synchronises the context's stream; the
 * dictionaries must outlive the launches.  Such batches, like those of cz_context_set_dictionary, take cz_decode_frames_kernel. */
#define CZ_MAX_DICTIONARIES 1024
int  cz_context_set_dictionaries(cz_context* ctx, const cz_dictionary* const* dicts, size_t k, const cz_dictionary* no_id_dict);

/* BlockDecoder (src/decoding/block_decoder.cairo:20-30): a plain value like the reference's struct. */
typedef struct cz_block_decoder {
    uint8_t internal_state;       /* DecoderState, block_decoder.cairo:26-30 */
    uint8_t header_buffer[3];
} cz_block_decoder;
#define CZ_BLOCK_READY_FOR_HEADER 0   /* ReadyToDecodeNextHeader */
#define CZ_BLOCK_READY_FOR_BODY   1   /* ReadyToDecodeNextBody */
#define CZ_BLOCK_FAILED           2   /* Failed (never set by the reference either, block_decoder.cairo:26-30) */
void cz_block_decoder_new(cz_block_decoder* bd);                                                   /* BlockDecoderTrait::new, :71-75 */
/* read_block_header (:237-278): *consumed = 3 once three bytes were there; moves the state to ReadyToDecodeNextBody. */
int  cz_block_decoder_read_block_header(cz_block_decoder* bd, const uint8_t* src, size_t len, cz_block_header* out, uint8_t* consumed);
/* decode_block_content (:77-137): decodes the body of the block `header` describes from src (positioned just behind the
 * header) into the workspace's DecodeBuffer, on the device.  *consumed = bytes of src the block took (Raw: its size,
 * RLE: 1, Compressed: content_size).  Errors: CZ_E_BLOCK_EXPECTED_HEADER / CZ_E_BLOCK_STATE_FAILED (state machine),
 * CZ_E_BH_RESERVED, or the DecompressBlockError leaf. */
int  cz_block_decoder_decode_block_content(cz_block_decoder* bd, const cz_block_header* header, cz_decoder_scratch* workspace,
                                           const uint8_t* src, size_t len, uint64_t* consumed);

/* ------------------------------------------- 3. resumable single-frame decoder */
/* FrameDecoder / FrameDecoderState (src/frame_decoder.cairo:17-30).  Source and target are
 * HOST buffers (as the reference's ByteArraySlice / ByteArray are); decoding runs on the
 * device, the decoded frame stays resident in HBM until collected. */
typedef struct cz_frame_decoder cz_frame_decoder;

typedef enum cz_strategy {          /* BlockDecodingStrategy, frame_decoder.cairo:33-37 */
    CZ_STRATEGY_ALL = 0,
    CZ_STRATEGY_UPTO_BLOCKS = 1,
    CZ_STRATEGY_UPTO_BYTES = 2
} cz_strategy;

int  cz_frame_decoder_create(cz_context* ctx, cz_frame_decoder** out);
void cz_frame_decoder_destroy(cz_frame_decoder* fd);
/* FrameDecoderStateTrait::new (frame_decoder.cairo:54-76): parses the frame header.
 * *consumed = header bytes; detail as cz_read_frame_header. */
int  cz_frame_decoder_new(cz_frame_decoder* fd, const uint8_t* src, size_t len, size_t* consumed, uint64_t* detail);
/* FrameDecoderStateTrait::reset (:78-104): same, plus the 100 MiB window cap (:92). */
int  cz_frame_decoder_reset(cz_frame_decoder* fd, const uint8_t* src, size_t len, size_t* consumed, uint64_t* detail);
uint64_t cz_frame_decoder_content_size(const cz_frame_decoder* fd);                 /* :125 */
int  cz_frame_decoder_checksum_from_data(const cz_frame_decoder* fd, uint32_t* v);  /* :129; returns 1 = Some */
uint32_t cz_frame_decoder_calculated_checksum(const cz_frame_decoder* fd);          /* :133-138 (low 32 bits of XXH64 of
                                                                                       the bytes drained so far) */
uint64_t cz_frame_decoder_bytes_read_from_source(const cz_frame_decoder* fd);       /* :140 */
int  cz_frame_decoder_is_finished(const cz_frame_decoder* fd);                      /* :144-150 */
size_t cz_frame_decoder_blocks_decoded(const cz_frame_decoder* fd);                 /* :152 */
/* decode_blocks (:156-222).  src points just past what earlier calls consumed.  *consumed =
 * bytes taken by this call, *finished = frame_finished. */
int  cz_frame_decoder_decode_blocks(cz_frame_decoder* fd, const uint8_t* src, size_t len, cz_strategy strategy,
                                    size_t n, size_t* consumed, int* finished);
size_t cz_frame_decoder_can_collect(const cz_frame_decoder* fd);                    /* :233-243 */
/* collect (:224-231).  Returns 1 = Some (bytes moved into dst, *written set), 0 = None,
 * <0 = -cz_status (dst too small: CZ_E_TARGET_TOO_SMALL). */
int  cz_frame_decoder_collect(cz_frame_decoder* fd, uint8_t* dst, size_t cap, size_t* written);
/* read (:328-334); returns bytes moved. */
size_t cz_frame_decoder_read(cz_frame_decoder* fd, uint8_t* dst, size_t cap);
/* FrameDecoderState.decoder_scratch (:25): the frame decoder's own DecoderScratch (owned by the frame decoder). */
cz_decoder_scratch* cz_frame_decoder_scratch(cz_frame_decoder* fd);
/* decode_from_to (:245-326): (*read_len, *written) = (source bytes consumed, target bytes produced). */
int  cz_frame_decoder_decode_from_to(cz_frame_decoder* fd, const uint8_t* src, size_t len, uint8_t* dst, size_t cap,
                                     size_t* read_len, size_t* written);


/* ------------------------------------------------------------- compression */
/*
 * Batched compression: n independent buffers become n standard zstd frames in one launch (cz_compress_frames_kernel,
 * DESIGN.md §10).  Any conforming decoder reads them.  The levels but one take greedy matches
 * from a hash table of 4-byte keys; CZ_COMPRESS_HIGH adds a second table, repeat-offset matches and a lazy parse.
 * Frame format: magic; Frame_Content_Size always written; Single_Segment when the input is at most 1 MiB, otherwise a
 * 1 MiB window (no offset exceeds it); no Dictionary_ID.  Blocks of at most 128 KiB, each Raw, RLE or Compressed,
 * whichever is smallest (an empty input: one empty last Raw block).  Literals Raw, RLE or Huffman (one stream below
 * 1 KiB of literals, four from 1 KiB, codes of at most 11 bits); sequences with the Predefined tables, or with
 * CZ_COMPRESS_FSE_TABLES the block's own.  A frame's bytes depend on its input bytes and `flags` alone, never on the batch
 * it was compressed in.
 */
/* Worst-case frame size for src_len bytes: frame header, a Raw block header per 128 KiB and the optional checksum. */
uint64_t cz_compress_bound(uint64_t src_len);
#define CZ_COMPRESS_CHECKSUM 1u     /* append the 4-byte XXH64 content checksum (Content_Checksum_flag) */
/*
 * CZ_COMPRESS_SPLIT (cz_compress_batch_device / _host only): an input longer than one segment of
 * cz_compress_split_segment() bytes (a multiple of 128 KiB) is cut into segments that different workgroups compress at the
 * same time.  The output is still ONE standard frame: the same header, blocks of at most 128 KiB each Raw, RLE or Compressed,
 * Last_Block on the final block only, the optional checksum of the whole input; cz_compress_bound still holds.  Matches reach
 * back into earlier segments (every segment after the first starts from the hash of the input bytes in front of it), and a
 * later segment writes its first offset explicitly.  The first segment comes out byte for byte as the first segment's worth
 * of the frame written without the flag.  An input of at most one segment comes out byte for byte as without the flag, and its
 * result flags do not carry CZ_COMPRESS_SPLIT; a split frame's do.  The bytes depend on the input and the flags alone, never on
 * the batch, the grid or timing.  A block that does not fit out_cap ends the frame with CZ_E_OUTPUT_TOO_SMALL as without the
 * flag: bytes_written / bytes_read / blocks cover the whole blocks placed, nothing past bytes_written is touched.
 * CZ_E_WAIT_EXPIRED: a segment waited for its predecessor beyond a bound of seconds (a fault of the library, not of the input);
 * the record then reports 0 bytes and the region's contents are unspecified.
 */
#define CZ_COMPRESS_SPLIT 4u
uint64_t cz_compress_split_segment(void);   /* the segment size S in bytes */
/*
 * CZ_COMPRESS_FSE_TABLES (cz_compress_batch_device / _host only, alone or with the two flags above): in every
 * Compressed block each of the literal-length, offset and match-length codes is written with Predefined_Mode, RLE_Mode (every
 * sequence of the block has the same code) or FSE_Compressed_Mode with a table made from the block's own histogram, whichever
 * makes the block smallest, compared by exact size (ties: Predefined, then RLE).  Repeat_Mode of an earlier table of the frame is
 * never written.  Everything else about the frame is as without the flag, so a frame without sequences comes out byte for byte
 * the same; cz_compress_bound still holds.  The result flags carry the bit whenever it was requested.  The value is 16: 8 stays an
 * unknown bit.  CZ_E_INVALID_ARG in cz_compress_batch_dict_*: dictionary frames use the dictionary's tables (Repeat) or the
 * Predefined ones, and mixing a dictionary's tables with the frame's own is left for later.
 */
#define CZ_COMPRESS_FSE_TABLES 16u
/*
 * CZ_COMPRESS_FAST (cz_compress_batch_device / _host only, alone or with CZ_COMPRESS_CHECKSUM): the fast level.
 * The frame header, the optional checksum and the limits are as without the flag; an empty input comes out byte for byte the same.
 * The input is cut into groups of 128 KiB and every group into sub-blocks of 32 KiB (the last of each may be shorter); every
 * sub-block becomes one block, Raw, RLE or Compressed, whichever is smallest (below 16 bytes: Raw or RLE), with the literal rules
 * above and the Predefined sequence tables, compressed by one wave on a hash table of its own.  Every block can be decoded without
 * any other block of the frame: no match reaches in front of its sub-block, Treeless literals and Repeat_Mode are never written, and
 * Offset_Value 1 only refers to an offset that an earlier sequence of the same block wrote explicitly.  A group whose blocks, headers
 * included, exceed 3 + its size is written as ONE Raw block of the group's size, so cz_compress_bound still holds although a frame may
 * hold four times as many blocks.  `blocks` counts the blocks written; CZ_E_OUTPUT_TOO_SMALL ends the frame at a group boundary
 * (bytes_written / bytes_read / blocks cover the whole groups placed, nothing past bytes_written is touched).  The bytes depend on
 * the input and the flags alone.  The result flags carry the bit whenever it was requested.  The value is 32: 8 stays an unknown bit.
 * CZ_E_INVALID_ARG together with CZ_COMPRESS_SPLIT or CZ_COMPRESS_FSE_TABLES and in cz_compress_batch_dict_*: these combinations
 * are left for later.
 */
#define CZ_COMPRESS_FAST 32u
/*
 * CZ_COMPRESS_RECORDS: the records level, for batches of very many small buffers, with or without dictionaries.
 * Every wave of the device takes a whole record and writes its whole frame; an input may be at most cz_compress_record_max() =
 * 32 KiB.  A longer one fails alone with CZ_E_INVALID_ARG: 0 bytes read and written, 0 blocks, its output region untouched.  The
 * frame header, the optional checksum and the limits are as without the flag (in cz_compress_batch_dict_* the Dictionary_ID rules
 * too); the frame has ONE block, Raw, RLE or Compressed, whichever is smallest (below 16 bytes: Raw or RLE; an empty input: one
 * empty last Raw block), so cz_compress_bound holds.  The bytes depend on the input, the dictionary and the flags alone.
 *   Without a dictionary (cz_compress_batch_device / _host, or CZ_COMPRESS_NO_DICT) the frame is byte for byte the CZ_COMPRESS_FAST
 * frame of the same input, and status, blocks, bytes_read and bytes_written are equal too.
 *   With a dictionary the matches come from the record itself (a table of 2^12 entries) and from the dictionary's content through
 * its prepared table, which is read where it lies and not copied; offsets reach 1 MiB.  The literals are Raw, RLE, Huffman or
 * Treeless with the dictionary's code, and each of LL / OF / ML is in Repeat_Mode with the dictionary's table when that has a state
 * for every code of the block, else Predefined.  The dictionary's three repeat offsets are not referred to.
 * Flags: in cz_compress_batch_device / _host alone or with CZ_COMPRESS_CHECKSUM; in cz_compress_batch_dict_* with
 * CZ_COMPRESS_CHECKSUM and / or CZ_COMPRESS_NO_DICT_ID.  CZ_E_INVALID_ARG together with CZ_COMPRESS_SPLIT, CZ_COMPRESS_FSE_TABLES or
 * CZ_COMPRESS_FAST.  The result flags carry the bit whenever it was requested.  The value is 64: 8 stays an unknown bit.
 */
#define CZ_COMPRESS_RECORDS 64u
uint64_t cz_compress_record_max(void);   /* 32768: the largest input CZ_COMPRESS_RECORDS takes */
/*
 * CZ_COMPRESS_FAST_SPLIT (cz_compress_batch_device / _host only, alone or with CZ_COMPRESS_CHECKSUM): the fast
 * level for few, large buffers.  The 128 KiB groups of one input are compressed by different workgroups at the same time, so one
 * buffer occupies the whole device.  For every input the frame is byte for byte the CZ_COMPRESS_FAST frame of the same input and
 * checksum flag, and status, blocks, bytes_read, bytes_written and checksum are equal too, for every out_cap: that includes
 * CZ_E_OUTPUT_TOO_SMALL where the header does not fit, where a group does not fit (the frame ends at that group boundary) and where
 * the 4 checksum bytes do not fit, and CZ_E_INVALID_ARG for an input of 0xFFF00000 bytes or more.  Only `flags` differs: it carries
 * 128 where the fast frame carries 32.  Nothing past bytes_written is touched.  The bytes depend on the input and the flags alone,
 * never on the batch, the grid or timing.  CZ_E_WAIT_EXPIRED is possible, as described for CZ_COMPRESS_SPLIT.  An input of at most
 * one group is one unit of work, as at the fast level: for batches of very many buffers of 128 KiB or less CZ_COMPRESS_FAST does
 * the same work without the plan launch and the search per unit.
 * The value is 128, a bit of its own (CZ_COMPRESS_FAST | CZ_COMPRESS_SPLIT stays CZ_E_INVALID_ARG; 8 stays an unknown bit).
 * CZ_E_INVALID_ARG together with any other flag but the checksum and in cz_compress_batch_dict_*.
 */
#define CZ_COMPRESS_FAST_SPLIT 128u
/*
 * CZ_COMPRESS_HIGH (cz_compress_batch_device / _host only, alone or with CZ_COMPRESS_CHECKSUM): the high-ratio
 * level.  Everything about the frame but the choice of sequences is the CZ_COMPRESS_FSE_TABLES frame, which the level implies: the
 * same header, blocks of at most 128 KiB each Raw, RLE or Compressed, the same literals, and per block and field Predefined, RLE
 * or FSE_Compressed mode by exact size; Repeat_Mode and Treeless literals are never written; cz_compress_bound holds,
 * CZ_E_OUTPUT_TOO_SMALL ends the frame at a block boundary with nothing past bytes_written touched, and an input of 0xFFF00000 bytes
 * or more is CZ_E_INVALID_ARG.  An input without any match (empty, below 16 bytes, an RLE block, random bytes) comes out byte for
 * byte as with CZ_COMPRESS_FSE_TABLES.  The sequences come from two candidates per position (the 4-byte table and a second table
 * of 8-byte keys that keeps long matches), from the offset history, which is tried as a match of its own and written with all six
 * repeat-offset cases of the format (an offset the history holds in a usable place is never written in full), and from a lazy
 * parse that gives up a short match for a longer one at one of the next two positions.  Offsets stay within 1 MiB.  The bytes
 * depend on the input and the flags alone, never on the batch, the grid or timing.  The result flags carry the bit whenever it was
 * requested.  The value is 256: 8 stays an unknown bit.  CZ_E_INVALID_ARG together with CZ_COMPRESS_SPLIT, CZ_COMPRESS_FSE_TABLES,
 * CZ_COMPRESS_FAST, CZ_COMPRESS_RECORDS or CZ_COMPRESS_FAST_SPLIT and in cz_compress_batch_dict_*: the split form of the level has
 * a flag of its own (CZ_COMPRESS_HIGH_SPLIT), the dictionary form is left for later.
 */
#define CZ_COMPRESS_HIGH 256u
/*
 * CZ_COMPRESS_HIGH_SPLIT (cz_compress_batch_device / _host only, alone or with CZ_COMPRESS_CHECKSUM): the
 * high-ratio level for few, large buffers.  An input longer than S = cz_compress_split_segment() bytes is cut into segments of S
 * bytes, which different workgroups compress at the same time into ONE standard frame.  The frame is CZ_COMPRESS_HIGH's in
 * everything but the sequences of later segments: the same header, blocks of at most 128 KiB each Raw, RLE or Compressed by size,
 * the same literals, per block and field Predefined, RLE or FSE_Compressed mode by exact size, never Repeat_Mode or Treeless
 * literals, Last_Block on the final block only; cz_compress_bound holds, offsets stay within 1 MiB, and an input of 0xFFF00000
 * bytes or more is CZ_E_INVALID_ARG.  An input of at most S bytes comes out byte for byte as with CZ_COMPRESS_HIGH; for a longer
 * one, segment 0 (the header and the blocks of the first S bytes) is byte for byte that frame's.  A later segment starts from
 * empty tables, into both of which the W input bytes in front of it are inserted (W as for CZ_COMPRESS_SPLIT; the 8-byte table
 * for positions with 8 bytes left in the input), so its matches reach back into the overlap and no further; and from an offset
 * history of (0, 0, 0), which equals no offset: its first sequence is written in full, and all six repeat-offset cases are used as
 * entries become known (what a segment knows is always a prefix of the decoder's history).  A block that is not written
 * Compressed leaves the history as it found it.  The bytes depend on the input and the flags alone, never on the batch, the grid
 * or timing.  CZ_E_OUTPUT_TOO_SMALL ends the frame at a block boundary: bytes_written, bytes_read and blocks cover the whole
 * blocks placed, and nothing past bytes_written is touched.  CZ_E_WAIT_EXPIRED is possible, as described for CZ_COMPRESS_SPLIT.
 * The result flags carry the bit whenever it was requested, whatever the input length.  An input of at most S bytes is one unit
 * of work: for batches of very many such buffers CZ_COMPRESS_HIGH does the same work without the plan launch and the search per
 * unit.
 * The value is 512, a bit of its own (CZ_COMPRESS_HIGH | CZ_COMPRESS_SPLIT stays CZ_E_INVALID_ARG; 8 stays an unknown bit).
 * CZ_E_INVALID_ARG together with any other flag but the checksum, CZ_COMPRESS_HIGH and CZ_COMPRESS_SPLIT included, and in
 * cz_compress_batch_dict_*.
 */
#define CZ_COMPRESS_HIGH_SPLIT 512u
/* One per buffer, written by the device. */
typedef struct cz_compress_result {
    int32_t  status;            /* CZ_OK | CZ_E_OUTPUT_TOO_SMALL | CZ_E_INVALID_ARG (an input of 4 GiB - 1 MiB or more) | CZ_E_WAIT_EXPIRED */
    uint32_t blocks;            /* blocks written */
    uint64_t bytes_read;        /* input bytes compressed into the blocks written */
    uint64_t bytes_written;     /* frame bytes at out_base + out_off[i]; nothing past them is touched */
    uint32_t checksum;          /* low 32 bits of XXH64 of the input when flags has CZ_COMPRESS_CHECKSUM */
    uint32_t flags;             /* the flags the frame was written with */
} cz_compress_result;
/* Compresses in_base[in_off[i] .. +in_len[i]) into out_base[out_off[i] .. +out_cap[i]) for every i < n.  DEVICE pointers
 * (results too); asynchronous on the context stream; no alignment required.  A frame that fails leaves its neighbours and
 * every byte of its own region past bytes_written untouched.  out_cap[i] = cz_compress_bound(in_len[i]) always suffices.
 * flags: CZ_COMPRESS_CHECKSUM, CZ_COMPRESS_SPLIT, CZ_COMPRESS_FSE_TABLES, CZ_COMPRESS_FAST (not with the two before it),
 * CZ_COMPRESS_RECORDS (not with the three before it), CZ_COMPRESS_FAST_SPLIT (with the checksum only), CZ_COMPRESS_HIGH (with the
 * checksum only), CZ_COMPRESS_HIGH_SPLIT (with the checksum only); any other bit is CZ_E_INVALID_ARG. */
int cz_compress_batch_device(cz_context* ctx, const void* d_in_base, const uint64_t* d_in_off, const uint64_t* d_in_len, size_t n,
                             void* d_out_base, const uint64_t* d_out_off, const uint64_t* d_out_cap, uint32_t flags,
                             cz_compress_result* d_results);
/* Same with HOST buffers: stages the inputs, compresses, copies outputs and results back, and synchronizes. */
int cz_compress_batch_host(cz_context* ctx, const void* in_base, size_t in_bytes, const uint64_t* in_off, const uint64_t* in_len, size_t n,
                           void* out_base, size_t out_bytes, const uint64_t* out_off, const uint64_t* out_cap, uint32_t flags,
                           cz_compress_result* results);

/*
 * Compression with dictionaries, the write side of cz_context_set_dictionaries: set the dictionaries once, then
 * run many batches.  A frame written with dictionary j names it by a Dictionary_ID field (1, 2 or 4 bytes, the smallest that holds
 * cz_dictionary_id; none for ID 0 or with CZ_COMPRESS_NO_DICT_ID), its matches may reach into the dictionary's content, its repeat
 * offsets start from the dictionary's three, and its first Compressed blocks may use the dictionary's Huffman code (Treeless
 * literals) and its LL / OF / ML tables (Repeat mode) while the frame has not replaced them.  Decode such frames with
 * cz_context_set_dictionaries (or cz_context_set_dictionary / init_from_dict).  cz_compress_bound still holds.
 */
#define CZ_COMPRESS_NO_DICT     0xFFFFFFFFu  /* dict_index entry: this frame is written without a dictionary */
#define CZ_COMPRESS_NO_DICT_ID  2u           /* flag: omit the Dictionary_ID field (like ZSTD_c_dictIDFlag = 0) */
/* The dictionaries later cz_compress_batch_dict_* calls on this context pick from (k == 0: none).  Prepares each dictionary for
 * compression the first time it is set (a hash table of its content and encode forms of its tables, kept with the dictionary and
 * freed by cz_dictionary_destroy).  CZ_E_INVALID_ARG when dicts is NULL with k > 0, an entry is NULL, a dictionary belongs to
 * another context, or k > CZ_MAX_DICTIONARIES; on any error the previous setting stays in force.  Independent of the decode
 * settings (cz_context_set_dictionary / _dictionaries).  Synchronises the context's stream; the dictionaries must outlive the launches. */
int cz_context_set_compress_dictionaries(cz_context* ctx, const cz_dictionary* const* dicts, size_t k);
/* As cz_compress_batch_device; frame i uses dicts[dict_index[i]] of the last cz_context_set_compress_dictionaries, or none for
 * CZ_COMPRESS_NO_DICT (the frame then comes out byte for byte as from cz_compress_batch_device).  Any other index >= k fails that
 * frame alone with CZ_E_INVALID_ARG (nothing written), as does a dictionary content plus input of 4 GiB - 1 MiB or more.
 * d_dict_index (DEVICE, n entries) may be NULL when exactly one dictionary is set: every frame uses it.  flags: CZ_COMPRESS_CHECKSUM,
 * CZ_COMPRESS_NO_DICT_ID, CZ_COMPRESS_RECORDS (CZ_COMPRESS_SPLIT, CZ_COMPRESS_FSE_TABLES and CZ_COMPRESS_FAST are CZ_E_INVALID_ARG here: split frames take
 * no dictionary, dictionary frames no tables of their own, and the fast level has no dictionary kernel: CZ_COMPRESS_RECORDS is that level for records of at most 32 KiB). */
int cz_compress_batch_dict_device(cz_context* ctx, const void* d_in_base, const uint64_t* d_in_off, const uint64_t* d_in_len, size_t n,
                                  void* d_out_base, const uint64_t* d_out_off, const uint64_t* d_out_cap, uint32_t flags,
                                  const uint32_t* d_dict_index, cz_compress_result* d_results);
/* Same with HOST buffers (dict_index too), as cz_compress_batch_host. */
int cz_compress_batch_dict_host(cz_context* ctx, const void* in_base, size_t in_bytes, const uint64_t* in_off, const uint64_t* in_len, size_t n,
                                void* out_base, size_t out_bytes, const uint64_t* out_off, const uint64_t* out_cap, uint32_t flags,
                                const uint32_t* dict_index, cz_compress_result* results);

/* ---- dictionary training ----
 * Makes a standard zstd dictionary from samples on the device: magic 0xEC30A437, Dictionary_ID, the Huffman description of the
 * literals, the FSE descriptions of OF, ML and LL, the repeat offsets 1, 4, 8, then the content.  The content is chosen as
 * fastCover chooses it (8-byte d-mers counted in 2^20 hashed counters; round after round the window of segment_len bytes with the
 * highest sum of counters, each d-mer once, from one of content_capacity / segment_len equal ranges of the samples; windows chosen
 * earlier lie nearer the end).  The tables come from parsing every sample against that content as cz_compress_batch_dict_* would;
 * every literal value and every LL (0..35), ML (0..52) and OF (0..20) code has a state, so libzstd takes the tables as valid and
 * this library's compressor writes Repeat_Mode with them.  When all samples together fit the content it is all of them, in order.
 * The bytes depend on the samples in their order, dict_cap and the parameters only.  dict_cap - 320 bytes are the content's room
 * (at most 1 GiB); *dict_len <= dict_cap, and no byte past *dict_len is written.
 * CZ_E_INVALID_ARG (nothing written): dict_cap < CZ_TRAIN_MIN_CAPACITY, n == 0, a non-zero reserved word, a segment_len outside
 * its range, 2 GiB of samples or more, no sample of 8 bytes or more, a NULL pointer other than params.
 * Synchronises the context's stream (training is set-up, like cz_context_measure_batch). */
typedef struct cz_train_params {
    uint32_t dict_id;      /* 0: 32768 + XXH64(content) % (2^31 - 32768), as ZDICT derives it */
    uint32_t segment_len;  /* 0: the default, CZ_TRAIN_SEGMENT; else 16 .. 4096 */
    uint32_t reserved[6];  /* must be 0 */
} cz_train_params;
#define CZ_TRAIN_SEGMENT 128
#define CZ_TRAIN_MIN_CAPACITY 1024
/* Samples: DEVICE pointers, laid out like a batch (base + off[] + len[]).  d_dict: DEVICE, dict_cap bytes.  params NULL: defaults. */
int cz_dictionary_train_device(cz_context* ctx, const void* d_base, const uint64_t* d_off, const uint64_t* d_len, size_t n,
                               void* d_dict, size_t dict_cap, const cz_train_params* params, size_t* dict_len);
/* Same with HOST buffers (bytes: the size of base; a sample outside it is CZ_E_INVALID_ARG). */
int cz_dictionary_train_host(cz_context* ctx, const void* base, size_t bytes, const uint64_t* off, const uint64_t* len, size_t n,
                             void* dict, size_t dict_cap, const cz_train_params* params, size_t* dict_len);
/* Milliseconds on the device of the last training's four steps: frequencies, epochs, statistics, tables and header. */
int cz_dictionary_train_last_ms(cz_context* ctx, float ms[4]);

/* ---- seekable streams ----
 * A batch of frames as ONE stream: the frames back to back, then one skippable frame, the seek table of the zstd seekable format,
 * that lists every frame's compressed and decompressed size (all fields little-endian, nothing aligned):
 *     frame 0 | ... | frame n-1 | 0x184D2A5E (4) | Frame_Size = n * E + 9 (4) | n entries of E bytes | footer (9)
 *     entry  = Compressed_Size (4), Decompressed_Size (4), [Checksum (4): low 32 bits of XXH64 of the decompressed bytes]
 *     footer = Number_Of_Frames (4), Seek_Table_Descriptor (1), 0x8F92EAB1 (4)
 * E is 8 without checksums and 12 with them.  Descriptor: bit 7 Checksum_Flag; bits 6..2 reserved, written as 0 and refused when
 * set; bits 1..0 unused, written as 0 and ignored.  Number_Of_Frames is at most CZ_SEEKABLE_MAX_FRAMES, and the frames listed cover
 * the stream from byte 0 to the table's first byte exactly.  Every zstd decoder reads such a stream (it skips the table; so do
 * cz_stream_split and cz_decode_stream); with the table, cutting the stream into a batch is two prefix sums, done on the device.
 */
#define CZ_SEEKABLE_CHECKSUMS 1u            /* flag: entries carry the checksum (cz_compress_result.checksum) */
#define CZ_SEEKABLE_MAX_FRAMES 0x8000000u
typedef struct cz_seekable_info {
    int32_t  status;        /* CZ_OK | CZ_E_SEEK_TABLE | CZ_E_INVALID_ARG | CZ_E_OUTPUT_TOO_SMALL */
    uint32_t reason;        /* CZ_E_SEEK_TABLE: the first check that failed, in the order below; else 0 */
    uint64_t frames;        /* Number_Of_Frames (pack: n) */
    uint64_t frames_bytes;  /* sum of Compressed_Size = offset of the seek table */
    uint64_t content_bytes; /* sum of Decompressed_Size over all frames */
    uint64_t stream_bytes;  /* frames_bytes + 8 + frames * E + 9 */
    uint64_t detail;
    uint32_t has_checksums, reserved;
} cz_seekable_info;
/* frame_bytes + 8 + n * E + 9: the stream of n frames of frame_bytes bytes together (flags: CZ_SEEKABLE_CHECKSUMS or 0). */
uint64_t cz_seekable_bound(uint64_t frame_bytes, size_t n, uint32_t flags);
/* Packs the output of any cz_compress_batch_* call as it lies: frame i is d_results[i].bytes_written bytes at d_frames_base +
 * d_frame_off[i], its Decompressed_Size is bytes_read, its Checksum is checksum.  All pointers are DEVICE pointers, d_info included.
 * Asynchronous on the context's stream and never synchronises: enqueued behind a compress launch of the same context it needs no
 * host step in between.  Returns CZ_E_INVALID_ARG for a flag bit other than CZ_SEEKABLE_CHECKSUMS, n above CZ_SEEKABLE_MAX_FRAMES or a
 * NULL pointer (n == 0: d_stream and d_info only are needed; the stream is the 17-byte table).  What depends on device data is decided on
 * the device (cz_seekable_plan_kernel) and reported in d_info->status:
 *   CZ_E_INVALID_ARG       a record with status != CZ_OK, with bytes_written or bytes_read of 2^32 or more, or (with
 *                          CZ_SEEKABLE_CHECKSUMS) with result flags that lack CZ_COMPRESS_CHECKSUM; detail = the lowest such index,
 *                          frames = n, the three sums are 0
 *   CZ_E_OUTPUT_TOO_SMALL  stream_bytes > stream_cap; stream_bytes and the other sums still report the need
 * On either error no byte of d_stream is touched; on success no byte past stream_bytes (and none in front of d_stream).  A frame's
 * slot is never read outside [0, bytes_written).  Source and stream must not overlap.  The bytes depend on the frames, their sizes
 * and flags alone. */
int cz_seekable_pack_device(cz_context* ctx, const void* d_frames_base, const uint64_t* d_frame_off, const cz_compress_result* d_results,
                            size_t n, void* d_stream, uint64_t stream_cap, uint32_t flags, cz_seekable_info* d_info);
/* Validates the table of the stream in HBM and writes, for frames [first, first + count), the four arrays that go into
 * cz_decode_batch_device unchanged (DEVICE pointers, count entries each): in_off absolute in the stream, in_len = Compressed_Size,
 * out_cap = Decompressed_Size, out_off = the exclusive sum of the range's out_cap each rounded up to out_align (the first frame of
 * the range at 0).  d_checksum (may be NULL) gets the entries' checksums, zeros when the table has none.  Any of the array pointers
 * may be NULL; with all five NULL the call only fills *info (the sizing call).  count == UINT64_MAX: up to the end.  `info` is a HOST
 * pointer; the call synchronises the context's stream (it is set-up, like cz_context_measure_batch) and returns info->status:
 *   CZ_E_INVALID_ARG  out_align not a power of two from 1 to 4096 or a NULL ctx / info / stream (decided on the host, nothing
 *                     launched), first > frames or first + count > frames (the table's fields are reported)
 *   CZ_E_SEEK_TABLE   reason = the first check that failed: 1 stream shorter than 17 bytes, 2 Seekable_Magic_Number wrong,
 *                     3 reserved descriptor bits set, 4 Number_Of_Frames above the maximum or a table longer than the stream,
 *                     5 Skippable_Magic_Number or Frame_Size at the computed table start wrong, 6 sum of Compressed_Size != table
 *                     offset; every other field of *info is 0
 * On any error no array is written.  info->detail = the output bytes the range needs (the last out_off plus the last out_cap; 0 for
 * an empty range). */
int cz_seekable_open_device(cz_context* ctx, const void* d_stream, uint64_t stream_len, uint64_t first, uint64_t count, uint32_t out_align,
                            uint64_t* d_in_off, uint64_t* d_in_len, uint64_t* d_out_off, uint64_t* d_out_cap, uint32_t* d_checksum,
                            cz_seekable_info* info);
/* The same two calls with HOST buffers and arrays, in plain C++ on the CPU (csrc/czstd_seekable_host.h; no device, no context, like
 * cz_stream_split): the library's second implementation of the format, which the kernels are held to.  Both return info->status. */
int cz_seekable_pack_host(const void* frames_base, const uint64_t* frame_off, const cz_compress_result* results, size_t n,
                          void* stream, uint64_t stream_cap, uint32_t flags, cz_seekable_info* info);
int cz_seekable_open_host(const void* stream, uint64_t stream_len, uint64_t first, uint64_t count, uint32_t out_align,
                          uint64_t* in_off, uint64_t* in_len, uint64_t* out_off, uint64_t* out_cap, uint32_t* checksum,
                          cz_seekable_info* info);

/* ---- byte ranges out of a seekable stream ----
 * "Content" is the frames' decompressed bytes in frame order, content_bytes of them; a range is (offset, length) in content
 * coordinates.  Reading m ranges is: an index of the stream (once), a locate (which frames hold a requested byte, and where each
 * range lies in their decode output), ONE cz_decode_batch_device of those k frames, and a gather of the ranges out of the decoded
 * frames into one destination, the ranges back to back.
 *
 * The index validates the table exactly as cz_seekable_open_device does (the same kernel; the same *info, with detail 0; on
 * CZ_E_SEEK_TABLE *out is NULL) and keeps in HBM the 64-bit scans of both size columns, the checksums and a per-frame scratch.
 * `info` is a HOST pointer; the call synchronises the context's stream.  The stream need not outlive the call.  CZ_E_INVALID_ARG for
 * a NULL ctx / out / info or a NULL stream with a length.  The index belongs to its context and is destroyed before it; calls on one
 * index are not to run side by side. */
typedef struct cz_seekable_index cz_seekable_index;
int  cz_seekable_index_create_device(cz_context* ctx, const void* d_stream, uint64_t stream_len, cz_seekable_index** out, cz_seekable_info* info);
void cz_seekable_index_destroy(cz_seekable_index* ix);
typedef struct cz_seekable_span {      /* one per range */
    uint64_t dst_off;     /* exclusive sum of the ranges' lengths, in range order: where its bytes go in the gather's destination */
    uint64_t src_off;     /* where its first byte lies in the decode output: out_off[sel_first] + (offset - content_off[sel_first]); 0 for an empty range */
    uint32_t sel_first;   /* index, among the selected frames, of the frame holding its first byte; 0 for an empty range */
    uint32_t sel_count;   /* selected frames it touches; 0 for an empty range */
} cz_seekable_span;                    /* 24 bytes */
typedef struct cz_seekable_read_info { /* 64 bytes */
    int32_t  status;        /* CZ_OK | CZ_E_INVALID_ARG | CZ_E_OUTPUT_TOO_SMALL (cz_seekable_locate_host also: CZ_E_SEEK_TABLE) */
    uint32_t reason;        /* device: reserved, written as 0 (the table was validated when the index was built); host: the table's defect */
    uint64_t frames, content_bytes;   /* of the table */
    uint64_t selected;      /* k: frames that hold at least one requested byte */
    uint64_t out_bytes;     /* decode output the k frames need at out_align: last out_off + last out_cap, 0 for k = 0 */
    uint64_t dst_bytes;     /* sum of the ranges' lengths */
    uint64_t detail;        /* a range outside the content: the lowest such index */
    uint32_t has_checksums, reserved;
} cz_seekable_read_info;
/* The selected frames are the union, over the m ranges (DEVICE arrays; they may overlap, repeat and come in any order), of the
 * frames with Decompressed_Size > 0 that hold a byte of the range, each once, in ascending frame number; an empty range selects
 * nothing and an empty frame is never selected.  Per selected frame s (DEVICE arrays of frames_cap entries, any of them NULL):
 * d_frame[s] its frame number, d_in_off / d_in_len / d_out_cap as cz_seekable_open_device gives them for that frame, d_out_off the
 * exclusive sum of the selected frames' sizes each rounded up to out_align, d_checksum[s] the table's checksum or 0,
 * d_content_off[s] the frame's first byte in content coordinates.  The first five go into cz_decode_batch_device unchanged, with
 * n = k.  d_spans (m entries, may be NULL): see cz_seekable_span; the selected frames of one range are consecutive.  With all eight
 * pointers NULL the call only fills *info (the sizing call).  `info` is a HOST pointer; the call synchronises and returns
 * info->status.  On any error no array is written and info carries the table's fields:
 *   CZ_E_INVALID_ARG       out_align not a power of two from 1 to 4096, a NULL ix / info, m above CZ_SEEKABLE_MAX_FRAMES, NULL
 *                          range arrays with m > 0 (decided on the host, nothing launched); a range with offset > content_bytes
 *                          or length > content_bytes - offset (decided on the device; detail = the lowest such index)
 *   CZ_E_OUTPUT_TOO_SMALL  k > frames_cap while a per-frame array is given; selected, out_bytes and dst_bytes still report
 * It reads the index, never the table again: O(m log n) for the ranges and passes over n 32-bit words for the selection.  The
 * results depend on the table, the ranges, out_align and frames_cap alone; the index's scratch is clean again when it returns. */
int cz_seekable_locate_device(cz_seekable_index* ix, const uint64_t* d_range_off, const uint64_t* d_range_len, size_t m,
                              uint32_t out_align, uint64_t frames_cap,
                              uint32_t* d_frame, uint64_t* d_in_off, uint64_t* d_in_len, uint64_t* d_out_off, uint64_t* d_out_cap,
                              uint32_t* d_checksum, uint64_t* d_content_off, cz_seekable_span* d_spans,
                              cz_seekable_read_info* info);
/* Copies range j's bytes out of the decoded frames (d_decoded + d_out_off[s]: what cz_decode_batch_device wrote for the k selected
 * frames) to d_dst + d_spans[j].dst_off: the destination is the ranges back to back, dst_bytes = info->dst_bytes of the locate.
 * All pointers are DEVICE pointers.  Asynchronous on the context's stream and never synchronises: it can sit directly behind the
 * decode launch.  No load leaves the bytes of a selected frame that a range asks for; no store leaves [0, dst_bytes), wherever
 * d_dst points.  m = 0 or dst_bytes = 0 launches nothing.  CZ_E_INVALID_ARG for a NULL ctx, m above CZ_SEEKABLE_MAX_FRAMES, or, with
 * bytes to copy, a NULL pointer or k = 0.  The arrays must be those of one locate: nothing here is checked on the device. */
int cz_seekable_gather_device(cz_context* ctx, const void* d_decoded, const uint64_t* d_out_off, const uint64_t* d_content_off, uint64_t k,
                              const uint64_t* d_range_off, const uint64_t* d_range_len, const cz_seekable_span* d_spans, size_t m,
                              void* d_dst, uint64_t dst_bytes);
/* The same on the CPU with HOST buffers and arrays (csrc/czstd_seekable_read_host.h, plain C++): the second implementation, which the
 * kernels are held to field for field and byte for byte.  cz_seekable_locate_host is stateless: it parses the table through
 * cz_seekable_open_host's validation each time (a damaged table: CZ_E_SEEK_TABLE with info->reason, every other field 0).
 * cz_seekable_gather_host also returns CZ_E_INVALID_ARG for a span that leaves [0, dst_bytes). */
int cz_seekable_locate_host(const void* stream, uint64_t stream_len, const uint64_t* range_off, const uint64_t* range_len, size_t m,
                            uint32_t out_align, uint64_t frames_cap,
                            uint32_t* frame, uint64_t* in_off, uint64_t* in_len, uint64_t* out_off, uint64_t* out_cap,
                            uint32_t* checksum, uint64_t* content_off, cz_seekable_span* spans, cz_seekable_read_info* info);
int cz_seekable_gather_host(const void* decoded, const uint64_t* out_off, const uint64_t* content_off, uint64_t k,
                            const uint64_t* range_off, const uint64_t* range_len, const cz_seekable_span* spans, size_t m,
                            void* dst, uint64_t dst_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CAIRO_ZSTD_AMD_H */
