/*
 * rrt_deflate.h -- C ABI of librrt_deflate.so: raw deflate streams (RFC 1951) made on the device from bytes that are on the device
 * already -- a PNG frame's filtered payload above all --, so that only finished streams cross PCIe and the host's threads are left
 * free.  A library of its own, as librrt_yuv.so, librrt_exr.so and librrt_png.so are: it needs nothing of the ray marcher or of the
 * PNG library and links no zlib; only rrt.h's status values are shared.
 *
 * Conventions (rrt.h's): every function returns an rrt_status; `d_*` pointers are DEVICE pointers owned by the caller; `stream` is a
 * hipStream_t passed as void* (NULL = the null stream).  A launch is a linear chain of THREE kernels on the caller's stream: no
 * allocation, no memset, no synchronisation, no hidden scratch -- it can be captured into a hipGraph.  Output, size table and
 * scratch are all the caller's.
 *
 * THE DEFINITION ("Device deflate"; tests/deflate_ref.py restates it)
 *
 *   Cuts.  The input is n bytes, cut into STREAMS of stream_bytes bytes; the last stream takes the rest.  Each stream is cut from its
 *   own start into SEGMENTS of RRT_DEFLATE_SEGMENT_BYTES bytes, the last one short.  An empty input is one stream of one empty
 *   segment.  A segment becomes one FRAGMENT: byte-aligned, independent of every other segment, without history.  A stream is the
 *   concatenation of its fragments.
 *
 *   The fragment of a segment b[0..m):
 *   1. Steps 2-8 are skipped when m = 0.
 *   2. Tokens, greedy, distance 1 only.  p = 0; while p < m: L = 0 if p = 0, otherwise the number of consecutive bytes from p on that
 *      equal b[p-1], capped at 258 and at the segment's end; L >= 3 emits match(L) and advances p by L, otherwise literal b[p] is
 *      emitted and p advances by 1.  Per maximal run of R equal bytes that is: one literal, (R-1) / 258 matches of 258, then the
 *      remainder (R-1) % 258 as one match if it is >= 3, otherwise as 1 or 2 literals.
 *   3. Counts over RFC 1951's 286 literal/length symbols; end-of-block counts 1; length 258 is symbol 285.
 *   4. lengths(counts, limit).  If exactly one symbol is used, the lowest-numbered unused symbol gets count 1.  Then repeat: sort the
 *      used symbols (the leaves) by (count, symbol) ascending; run the two-queue Huffman merge -- internal nodes queue up in order of
 *      creation, and when the two queue heads weigh the same the leaf is taken --; a leaf's length is its depth; if the greatest
 *      length exceeds `limit`, every non-zero count c becomes (c + 1) >> 1 and the merge is done again.
 *   5. Codes: canonical, RFC 1951 section 3.2.2, bit-reversed into the LSB-first stream.
 *   6. Block header: BFINAL 0, BTYPE 2; HLIT = nll - 257 with nll = max(257, highest used symbol + 1); HDIST = 1: two distance codes,
 *      both of length 1, always (distance 1 is the single bit 0; the code is complete).  The sequence ll[0..nll) + [1, 1] is
 *      run-length coded as ONE sequence over its maximal runs of equal values: a run of zeros -- while the run is >= 11, symbol 18
 *      for min(run, 138); then symbol 17 if 3 or more remain; then the rest as zeros --; a run of a non-zero v -- v once; then
 *      while 3 or more remain, symbol 16 for min(rest, 6); then the rest as v.  The 19 code-length symbols are counted and given
 *      lengths(., 7); HCLEN = ncl - 4 with ncl = max(4, last non-zero in the RFC's permuted order + 1).
 *   7. Body: the tokens, then end-of-block.
 *   8. Stored fallback.  D = ceil((bits of steps 6-7 + 3) / 8) + 4.  If D >= m + 10 the block is instead a stored block: BFINAL 0,
 *      BTYPE 0, pad, LEN, NLEN, the m bytes.
 *   9. Trailer: an empty stored block -- one bit F, BTYPE 00, pad to the byte, 00 00 FF FF.  F = 1 only on the last segment of the
 *      last stream, and only when the caller asks for `finish`; every other fragment ends as a sync flush does.
 *
 *   A fragment is therefore at most m + 10 bytes (5 when m = 0).
 *
 *   Refusals (RRT_ERR_INVALID_ARGUMENT before any device call, a message in rrt_deflate_last_error): NULL pointers; n >= 2^32;
 *   stream_bytes < 1; an out_bound of 2^32 bytes or more; outputs that overlap the input or each other; d_stream_sizes not 4-byte
 *   aligned; d_scratch not 16-byte aligned.
 */
#ifndef RRT_DEFLATE_H
#define RRT_DEFLATE_H

#include <stddef.h>
#include <stdint.h>

#include "rrt.h"     /* rrt_status */

#ifdef __cplusplus
extern "C" {
#endif

#define RRT_DEFLATE_SEGMENT_BYTES 32768      /* a segment: the bytes one fragment holds and one workgroup codes */
#define RRT_DEFLATE_THREADS 256              /* that workgroup */
#define RRT_DEFLATE_CHUNK_BYTES 128          /* consecutive input bytes per thread of it */
#define RRT_DEFLATE_LL_SYMBOLS 286           /* RFC 1951's literal/length alphabet */
#define RRT_DEFLATE_MAX_SYMBOLS 288          /* the most symbols rrt_deflate_code_lengths_host takes */

/* The cut and the buffers of a call: streams, segments, the worst case of step 8 (n + 10 per non-empty segment, 5 per empty one:
 * what d_out must hold) and the bytes of scratch a launch needs.  Host only; any of the four outputs may be NULL. */
int rrt_deflate_plan(size_t n, size_t stream_bytes, size_t* n_streams, size_t* n_segments, size_t* out_bound, size_t* scratch_bytes);

/* How a launch of this size is laid out, for tests and tools.  `address_bits`: the input's address (only the low four bits are looked
 * at; 0 stands for a 16-byte aligned buffer).
 *   out[0] threads, out[1] workgroups, out[2] bytes of LDS of deflate_segments (a workgroup per segment);
 *   out[3], out[4], out[5] the same of deflate_offsets (one workgroup: the prefix sum of the fragment lengths, the stream sizes);
 *   out[6], out[7], out[8] the same of deflate_gather (a workgroup per segment: the byte-exact compaction);
 *   out[9] bytes at the input's start that are loaded one by one (the part of a 16-byte word that lies inside the buffer),
 *   out[10] the same at its end, out[11] the 16-byte loads of the whole input (0: the byte path alone).
 * Host only. */
int rrt_deflate_launch_geometry(size_t n, size_t stream_bytes, size_t address_bits, int32_t out[12]);

/* Step 4 on its own: lengths_out[0..n_symbols) from counts[0..n_symbols), 2 <= n_symbols <= RRT_DEFLATE_MAX_SYMBOLS,
 * 1 <= limit <= 15 and 2^limit >= n_symbols; *halvings (may be NULL) receives how often the counts were halved.  Counts that are
 * all zero give lengths that are all zero.  Host only, from the source the kernels run. */
int rrt_deflate_code_lengths_host(const uint32_t* counts, int n_symbols, int limit, uint8_t* lengths_out, int32_t* halvings);

/* The definition on the device: d_out receives the streams back to back, compacted (at most out_bound bytes; nothing beyond the
 * streams' total is written), d_stream_sizes one uint32 per stream, both from d_src's n bytes (d_src may be NULL when n = 0).
 * d_scratch: scratch_bytes bytes, 16-byte aligned; its contents before and after are meaningless -- another launch's leftovers are
 * as good as any.  d_out and d_src need no alignment; no byte in front of d_out is written.  finish: 0 | 1, step 9's F. */
int rrt_launch_deflate(void* d_out, uint32_t* d_stream_sizes, void* d_scratch, const void* d_src, size_t n, size_t stream_bytes, int finish, void* stream);

/* The same bytes and sizes on HOST memory, from the source the kernels run; *total (may be NULL) receives the streams' bytes */
int rrt_deflate_host(void* out, uint32_t* stream_sizes, const void* src, size_t n, size_t stream_bytes, int finish, size_t* total);

/* Why the last call on this thread was refused ("" after a call that was not) */
const char* rrt_deflate_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
