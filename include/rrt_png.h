/*
 * rrt_png.h -- C ABI of librrt_png.so: a finished frame as the filtered scanlines of a PNG file, 8 or 16 bits per sample, on the
 * device, so that only the bytes deflate reads cross PCIe and the host never filters, scores or sums a scanline.  A library of its
 * own, as librrt_yuv.so and librrt_exr.so are: it needs nothing of the ray marcher and include/rrt.h is unchanged by it; only rrt.h's
 * status values are shared.  It does not deflate and links no zlib: its CRCs come from a table of its own.
 *
 * Conventions (rrt.h's): every function returns an rrt_status; `d_*` pointers are DEVICE pointers owned by the caller; `stream` is a
 * hipStream_t passed as void* (NULL = the null stream).  A launch is ONE kernel on the caller's stream: no allocation, no memset,
 * no synchronisation, no scratch -- it can be captured into a hipGraph.  Payload and row sums are both the caller's.
 *
 * THE DEFINITION ("PNG output")
 *
 *   The frame is width x height, buffer rows bottom-up: PNG row r (0 = top) is buffer row height - 1 - r.  Colour type 2 (RGB): no
 *   alpha, no interlace, no palette.
 *
 *   1. Samples.  Depth 8, from the RGBA8 frame: the bytes R, G, B as they are (alpha is ignored).  Depth 16, from the float4 linear
 *      HDR (rrt_debug_outputs.d_hdr, the `lin` output of the _ss launches, what rrt_launch_exposure leaves): q_c of "Y4M output",
 *      step 1 -- yuv_q_from_hdr of csrc/rrt_yuv_core.h, the tone map at 16 bits: NaN and negatives 0 --, two bytes, most significant
 *      first.  A raw scanline is width * bpp bytes, bpp = 3 | 6.
 *   2. Filters: the PNG specification's five, byte-wise; `a` the raw byte bpp to the left (0 in the first pixel), `b` the raw byte
 *      above, `c` above-left; the row above row 0 is all zeros.  A filter always reads RAW bytes.
 *        0 None x   1 Sub x - a   2 Up x - b   3 Average x - ((a + b) >> 1)
 *        4 Paeth x - P: p = a + b - c, P the first of a, b, c, in that order, whose distance to p is smallest.   All mod 256.
 *   3. Choice.  RRT_PNG_ADAPTIVE: each of the five candidates is scored by the sum over the row's width * bpp filtered bytes of
 *      v < 128 ? v : 256 - v (the type byte is not scored); the smallest score wins, ties go to the lowest type number.  A fixed
 *      filter applies to every row, row 0 included.
 *   4. Payload: height rows of stride = 1 + width * bpp bytes, tightly packed: the type byte, then the filtered bytes.  The zlib
 *      stream's input, byte for byte.
 *   5. Row sums: per row two uint32, s1 = sum d_i mod 65521 and s2 = sum (stride - i) d_i mod 65521 over the row's `stride` bytes
 *      d_0 ... (the type byte included).  The stream's Adler-32 follows in O(height) (rrt_png_adler32): A = 1, B = 0; per row
 *      B = (B + s2 + stride * A) mod 65521, then A = (A + s1) mod 65521; the result is B << 16 | A.
 *   6. File: the signature, IHDR, sRGB (intent 0), tEXt Software (rrt_png_header's bytes), the IDAT chunks, IEND.  The payload is cut
 *      into slices of R = ceil(2^20 / stride) rows (rrt_png_slices), the last may be short; each slice is deflated on its own as a
 *      raw stream (window -15) that ends with a sync flush, the last slice's with a finish; one IDAT per slice, the first prefixed
 *      with the two zlib header bytes 0x78 0x01, the last followed by the Adler-32, big-endian.  The cut depends on the frame alone.
 *   7. Refusals (RRT_ERR_INVALID_ARGUMENT before any device call, a message in rrt_png_last_error): NULL pointers; a struct_size,
 *      depth or filter off the lists; width or height < 1; width * height >= 2^31; a payload of 2^32 bytes or more; an output that
 *      overlaps the input; a depth that is not the entry point's (8 from RGBA8, 16 from the HDR).
 */
#ifndef RRT_PNG_H
#define RRT_PNG_H

#include <stddef.h>
#include <stdint.h>

#include "rrt.h"     /* rrt_status */

#ifdef __cplusplus
extern "C" {
#endif

#define RRT_PNG_NONE 0           /* the file format's own filter type numbers */
#define RRT_PNG_SUB 1
#define RRT_PNG_UP 2
#define RRT_PNG_AVERAGE 3
#define RRT_PNG_PAETH 4
#define RRT_PNG_ADAPTIVE 5       /* step 3's choice, row by row */

#define RRT_PNG_SLICE_BYTES 1048576      /* step 6: a slice is the fewest rows that hold this many bytes */
#define RRT_PNG_BAND_ROWS 4              /* the wide path: consecutive rows one workgroup filters */
#define RRT_PNG_SEGMENT_CHUNKS 2024      /* the wide path: 16-byte chunks of a row staged in LDS at a time; a longer row is cut */

typedef struct rrt_png_format {
    uint32_t struct_size;    /* sizeof(rrt_png_format): rrt_png_format_default sets it; any other value is RRT_ERR_INVALID_ARGUMENT */
    int32_t depth;           /* 8 | 16 */
    int32_t filter;          /* RRT_PNG_NONE ... RRT_PNG_PAETH: that filter on every row | RRT_PNG_ADAPTIVE */
} rrt_png_format;

/* 8, RRT_PNG_ADAPTIVE */
int rrt_png_format_default(rrt_png_format* fmt);

/* Step 4's byte count, the stride and the bytes of the row-sum table (8 per row).  Host only; stride and row_sum_bytes may be NULL. */
int rrt_png_frame_bytes(const rrt_png_format* fmt, int width, int height, size_t* payload_bytes, size_t* stride, size_t* row_sum_bytes);

/* Step 6's cut: rows per slice and the number of slices.  Host only. */
int rrt_png_slices(const rrt_png_format* fmt, int width, int height, int32_t* rows_per_slice, int32_t* n_slices);

/* How a launch of this size is laid out, for tests and tools.  `address_bits`: the bitwise OR of the payload's and the input's
 * addresses (only the low four bits are looked at; 0 stands for 16-byte aligned buffers).
 *   out[0] threads per workgroup, out[1] rows per workgroup (wide: the band, RRT_PNG_BAND_ROWS; narrow: one row per thread),
 *   out[2] workgroups (a one-dimensional grid), out[3] the most 16-byte chunks a row's span touches, out[4] the segments a row is
 *   staged in (> 1: a row longer than the staging), out[5] bytes of dynamic LDS, out[6] 1 wide | 0 narrow, out[7] chunks per segment.
 * Wide: both buffers 16-byte aligned, at any width.  Host only. */
int rrt_png_launch_geometry(const rrt_png_format* fmt, int width, int height, size_t address_bits, int32_t out[8]);

/* Steps 1-5 on the device: d_payload receives rrt_png_frame_bytes bytes, d_row_sums two uint32 per row.  Refused as step 7 says and:
 * d_row_sums or d_hdr not 4-byte aligned; d_row_sums overlapping the payload or the input. */
int rrt_launch_png_from_rgba8(void* d_payload, uint32_t* d_row_sums, const void* d_rgba8, int width, int height, const rrt_png_format* fmt, void* stream);
int rrt_launch_png_from_hdr(void* d_payload, uint32_t* d_row_sums, const float* d_hdr, int width, int height, const rrt_png_format* fmt, void* stream);

/* The same bytes and sums on HOST memory, from the source the kernels run */
int rrt_png_from_rgba8_host(void* payload, uint32_t* row_sums, const void* rgba8, int width, int height, const rrt_png_format* fmt);
int rrt_png_from_hdr_host(void* payload, uint32_t* row_sums, const float* hdr, int width, int height, const rrt_png_format* fmt);

/* The inverse of steps 2-4: `raw` receives height rows of width * bpp raw bytes, top-down, from a payload whose rows name their own
 * filter types (fmt->filter is not looked at).  A type byte above 4 is refused.  Host only. */
int rrt_png_unfilter_host(void* raw, const void* payload, int width, int height, const rrt_png_format* fmt);

/* Step 5's fold of a HOST row-sum table into the stream's Adler-32 */
int rrt_png_adler32(const uint32_t* row_sums, int width, int height, const rrt_png_format* fmt, uint32_t* adler);

/* The file's bytes from the signature through tEXt, CRCs included; the IDAT chunks follow.  `cap` smaller than that is refused. */
int rrt_png_header(const rrt_png_format* fmt, int width, int height, void* buf, size_t cap, size_t* len);

/* Why the last call on this thread was refused ("" after a call that was not) */
const char* rrt_png_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
