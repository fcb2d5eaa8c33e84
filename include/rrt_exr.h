/*
 * rrt_exr.h -- C ABI of librrt_exr.so: the frame's linear HDR packed as the scanline chunks of an OpenEXR file, half or float, on
 * the device, so that only the bytes the file holds cross PCIe.  A library of its own, as librrt_yuv.so is: it needs nothing of the
 * ray marcher and include/rrt.h is unchanged by it; only rrt.h's status values are shared.  It does not deflate and links no zlib:
 * with ZIPS or ZIP it leaves the chunk filtered, and the caller is left with nothing but deflate.
 *
 * Conventions (rrt.h's): every function returns an rrt_status; `d_*` pointers are DEVICE pointers owned by the caller; `stream` is a
 * hipStream_t passed as void* (NULL = the null stream).  A launch is ONE kernel on the caller's stream: no allocation, no memset,
 * no synchronisation, no scratch -- it can be captured into a hipGraph.
 *
 * THE DEFINITION ("EXR output")
 *
 *   The source is the frame's float4 HDR plane, width x height, rows bottom-up (rrt_debug_outputs.d_hdr, the `lin` output of the
 *   _ss launches, what rrt_launch_exposure leaves).  The file is top-down: EXR row y is source row height - 1 - y.  Alpha is not
 *   stored.
 *
 *   1. Samples.  FLOAT: the binary32 bits as they are (NaN and inf included: the caller chose a format that holds them).
 *      HALF: binary32 -> binary16, round to nearest even, subnormal halves kept, in integer arithmetic (exr_half_bits,
 *      csrc/rrt_exr_core.h).  NaN becomes +0.  A finite magnitude that rounds above half_max, and +-inf, become +-half_max: the
 *      file never holds an inf or a NaN that this conversion made.  -0 stays -0.
 *   2. Chunks.  NONE and ZIPS: 1 scanline per chunk; ZIP: 16, the last chunk may be short.  Chunk i starts at row y = i * lines.
 *      A scanline is the width samples of B, then of G, then of R (the file's alphabetical channel order), little-endian; a
 *      chunk's raw bytes are its scanlines top-down, n = rows * width * 3 * (2 | 4) bytes, always even.
 *   3. Filter (ZIPS and ZIP only; the format's reversible step in front of deflate), per chunk:
 *        tmp[0 .. n/2) = raw bytes at even offsets, tmp[n/2 .. n) = raw bytes at odd offsets;
 *        out[0] = tmp[0], out[j] = (tmp[j] - tmp[j-1] + 128) mod 256 for j >= 1 -- across the seam at n/2 too.
 *      Every output byte depends on two samples only.
 *   4. Payload: the chunks' bytes (raw with NONE, filtered otherwise) one behind the other, chunk i at `offset` of rrt_exr_chunk;
 *      width * height * 3 * (2 | 4) bytes in all.
 *   5. File (single part, scanline, version 2, no flags): rrt_exr_header's bytes; the offset table, one uint64 per chunk (the
 *      chunk's position from the start of the file); the chunks, each int32 y, int32 size, data.  With ZIPS / ZIP the data is
 *      the deflated (zlib stream) filtered chunk, or -- when that is not smaller than n -- the RAW chunk (rrt_exr_unfilter_host
 *      gives it back), which a reader recognises by size == n.
 */
/*
 * DATA LAYERS ("EXR data layers"): per-ray planes next to B, G, R, as further channels of the same scanlines
 *
 *   A layered frame is described by one rrt_exr_layers: the compression and half_max of rrt_exr_format, up to RRT_EXR_MAX_SOURCES
 *   sources and up to RRT_EXR_MAX_CHANNELS channels.
 *
 *   A source is a device plane of width x height pixels, `words` (1, 3 or 4) 32-bit words per pixel, 4-byte aligned, of binary32
 *   (RRT_EXR_SRC_F32) or int32 (RRT_EXR_SRC_I32) values.  bottom_up = 1: EXR row y is source row height - 1 - y (the HDR plane);
 *   0: row y (rrt_debug_outputs' d_rad, d_pos, d_vel, d_steps, d_hit).
 *
 *   A channel is a name -- 1 to 31 bytes of [A-Za-z0-9_.], neither starting nor ending with '.' --, the stored type (RRT_EXR_UINT,
 *   HALF or FLOAT: the file's codes), a source and a word of that source's pixel.  Channels arrive in strictly ascending strcmp
 *   order (unsigned bytes): the order the file stores them, so "channel i" means one thing everywhere.  Unsorted or duplicate names
 *   are refused, with the offending pair in rrt_exr_last_error.
 *
 *   1'. Samples (exr_layer_sample, csrc/rrt_exr_core.h):
 *         F32 -> FLOAT  the bits as they are            I32 -> UINT   the value; a negative value becomes 0
 *         F32 -> HALF   step 1's conversion             I32 -> FLOAT  (float)v, round to nearest even
 *         F32 -> UINT   refused                         I32 -> HALF   (float)v, then step 1's conversion
 *   2'. A scanline is the channels in order, each `width` samples of 2 (HALF) or 4 (FLOAT, UINT) bytes, little-endian; chunks of 1
 *       or 16 scanlines as in step 2; a chunk's raw bytes are n = rows * width * (the sum of the channels' sample sizes).
 *   3'. Step 3 as it is, byte-wise over the whole chunk.  With mixed sample sizes the predecessor of a channel's first sample in a
 *       row is the LAST TWO BYTES of the previous channel's last sample, whatever its type (exr_layer_tail).
 *   4', 5'. As steps 4 and 5; rrt_exr_layers_header writes rrt_exr_header's attributes in its order with the layers' channel list
 *       (pLinear 0, samplings 1, 1).
 *
 *   The layer set {B, G, R} from one bottom-up 4-word F32 source, words 2, 1, 0, gives the payload, chunk table and header of
 *   rrt_launch_exr_from_hdr, rrt_exr_from_hdr_host and rrt_exr_header byte for byte, in all six formats.
 */
#ifndef RRT_EXR_H
#define RRT_EXR_H

#include <stddef.h>
#include <stdint.h>

#include "rrt.h"     /* rrt_status */

#ifdef __cplusplus
extern "C" {
#endif

#define RRT_EXR_HALF 1           /* the file format's own pixel-type codes */
#define RRT_EXR_FLOAT 2
#define RRT_EXR_NONE 0           /* ... and its compression codes */
#define RRT_EXR_ZIPS 2
#define RRT_EXR_ZIP 3

typedef struct rrt_exr_format {
    uint32_t struct_size;    /* sizeof(rrt_exr_format): rrt_exr_format_default sets it; any other value is RRT_ERR_INVALID_ARGUMENT */
    int32_t type;            /* RRT_EXR_HALF | RRT_EXR_FLOAT */
    int32_t compression;     /* RRT_EXR_NONE | RRT_EXR_ZIPS | RRT_EXR_ZIP */
    float half_max;          /* HALF: the largest magnitude written; a finite positive half (65504, the largest, by default) */
} rrt_exr_format;

/* HALF, ZIP, 65504 */
int rrt_exr_format_default(rrt_exr_format* fmt);

/* Step 4's byte count and the number of chunks.  Host only; n_chunks may be NULL.  RRT_ERR_INVALID_ARGUMENT (every function below
 * refuses these the same way, with a message in rrt_exr_last_error): NULL pointers, a struct_size, type or compression outside the
 * lists, a half_max that is not a finite positive half, width or height < 1, a chunk of 2^31 bytes or more. */
int rrt_exr_frame_bytes(const rrt_exr_format* fmt, int width, int height, size_t* payload_bytes, int32_t* n_chunks);

/* Chunk i: its first row y, its byte offset in the payload, its (raw = filtered) size.  Host only; i outside [0, n_chunks) is
 * refused. */
int rrt_exr_chunk(const rrt_exr_format* fmt, int width, int height, int i, int32_t* y, size_t* offset, size_t* bytes);

/* How a launch of this size is laid out, for tests and tools.  `address_bits`: the bitwise OR of the payload's and the HDR plane's
 * addresses (only the low four bits are looked at; 0 stands for 16-byte aligned buffers).
 *   out[0] threads per workgroup, out[1] x out[2] its shape (x: along a row, y: rows),
 *   out[3] pixels of a row one thread packs: 8 on the wide path; 1 on the narrow path, where a thread packs ONE sample of a pixel,
 *   out[4] x out[5] the grid, out[6] 1 wide | 0 narrow, out[7] the passes a workgroup makes over the rows: ceil(height /
 *   (out[2] * out[5])), > 1 where the grid's row dimension wraps.
 * Wide: width % 8 == 0 and both buffers 16-byte aligned, so that every row of every channel starts on 16 bytes.  Host only. */
int rrt_exr_launch_geometry(const rrt_exr_format* fmt, int width, int height, size_t address_bits, int32_t out[8]);

/* Steps 1-4 on the device: d_payload receives rrt_exr_frame_bytes bytes.  Refused before any device call, as above and: d_hdr not
 * 4-byte aligned, an output that overlaps the input.  A d_payload or d_hdr that is not 16-byte aligned is served by the narrow path. */
int rrt_launch_exr_from_hdr(void* d_payload, const float* d_hdr, int width, int height, const rrt_exr_format* fmt, void* stream);

/* The same bytes on HOST memory, from the source the kernels run (no device is touched) */
int rrt_exr_from_hdr_host(void* payload, const float* hdr, int width, int height, const rrt_exr_format* fmt);

/* Step 3's inverse: the raw bytes of a filtered chunk of n bytes (n even, 2 <= n < 2^31; raw and filtered must not overlap).  For
 * the chunks that deflate does not shrink.  Host only. */
int rrt_exr_unfilter_host(void* raw, const void* filtered, size_t n);

/* Step 5's header into buf[0 .. cap): magic, version, the eight required attributes (channels, compression, dataWindow,
 * displayWindow, lineOrder = INCREASING_Y, pixelAspectRatio = 1, screenWindowCenter = (0, 0), screenWindowWidth = 1), then
 * chromaticities (BT.709 primaries, D65 white), framesPerSecond (the rational fps_num / fps_den) and software, and the closing 0.
 * *len is its length; the offset table starts there.  Host only.  Also refused: fps_num or fps_den <= 0, a cap too small (nothing
 * is written then). */
int rrt_exr_header(const rrt_exr_format* fmt, int width, int height, int fps_num, int fps_den, void* buf, size_t cap, size_t* len);

/* ---- data layers (the second block comment above) ---- */

#define RRT_EXR_UINT 0           /* the file format's third pixel type */
#define RRT_EXR_SRC_F32 0        /* a source's words: binary32 ... */
#define RRT_EXR_SRC_I32 1        /* ... or int32 */
#define RRT_EXR_MAX_SOURCES 8
#define RRT_EXR_MAX_CHANNELS 16

typedef struct rrt_exr_source {
    const void* d_data;      /* width * height * words 32-bit words; a DEVICE pointer for the launch, a host pointer for rrt_exr_layers_host */
    int32_t words;           /* 32-bit words per pixel: 1 | 3 | 4 */
    int32_t kind;            /* RRT_EXR_SRC_F32 | RRT_EXR_SRC_I32 */
    int32_t bottom_up;       /* 1: EXR row y is source row height - 1 - y; 0: row y */
    int32_t reserved;        /* 0 */
} rrt_exr_source;

typedef struct rrt_exr_channel {
    char name[32];           /* NUL-terminated, 1 ... 31 bytes */
    int32_t type;            /* RRT_EXR_UINT | RRT_EXR_HALF | RRT_EXR_FLOAT */
    int32_t source;          /* an index into sources */
    int32_t word;            /* < that source's words */
    int32_t reserved;        /* 0 */
} rrt_exr_channel;

typedef struct rrt_exr_layers {
    uint32_t struct_size;    /* sizeof(rrt_exr_layers): rrt_exr_layers_default sets it; any other value is RRT_ERR_INVALID_ARGUMENT */
    int32_t compression;     /* RRT_EXR_NONE | RRT_EXR_ZIPS | RRT_EXR_ZIP */
    float half_max;          /* as rrt_exr_format's */
    int32_t n_sources;       /* 1 ... RRT_EXR_MAX_SOURCES */
    int32_t n_channels;      /* 1 ... RRT_EXR_MAX_CHANNELS */
    int32_t reserved;        /* 0 */
    rrt_exr_source sources[RRT_EXR_MAX_SOURCES];
    rrt_exr_channel channels[RRT_EXR_MAX_CHANNELS];
} rrt_exr_layers;

/* zero sources and channels, ZIP, 65504 */
int rrt_exr_layers_default(rrt_exr_layers* layers);

/* rrt_exr_frame_bytes and rrt_exr_chunk for a layered frame.  Host only; the sources' d_data are not looked at.  Refused like a
 * format and: n_sources or n_channels outside their ranges, a source's words or kind outside the lists, a channel name that breaks
 * the rule, names not strictly ascending, a type outside the list, a source or word out of range, an F32 source stored as UINT, a
 * chunk of 2^31 bytes or more. */
int rrt_exr_layers_frame_bytes(const rrt_exr_layers* layers, int width, int height, size_t* payload_bytes, int32_t* n_chunks);
int rrt_exr_layers_chunk(const rrt_exr_layers* layers, int width, int height, int i, int32_t* y, size_t* offset, size_t* bytes);

/* out[8] with the meanings of rrt_exr_launch_geometry; `address_bits`: the OR of the payload's and every source's address.
 *   Narrow (out[6] = 0): a thread packs ONE sample; out[4] covers width * n_channels threads along a row.
 *   Wide (out[6] = 1 | 2): width % 8 == 0, the payload and every source 16-byte aligned.  A thread packs 8 pixels of a row: it reads
 *   each source once, in 16-byte loads, and stores 16 bytes per channel (HALF, raw), 2 x 16 (FLOAT / UINT, raw) or -- filtered --
 *   one store into each half of the chunk, 8 bytes for HALF and 16 for FLOAT / UINT.  A channel's place in each half of a filtered
 *   chunk is a multiple of 8 only: width x (half the sample bytes of the rows and channels in front).  So where a filtered layout
 *   holds both a HALF and a 4-byte channel and width % 16 == 8, EVERY 4-byte channel is stored in 8-byte stores, two into each
 *   half: out[6] = 2.  Every other wide layout (raw rows always) is 16-byte aligned throughout: out[6] = 1. */
int rrt_exr_layers_launch_geometry(const rrt_exr_layers* layers, int width, int height, size_t address_bits, int32_t out[8]);

/* Steps 1'-4' on the device: ONE kernel on `stream`, no allocation, memset, synchronisation or scratch.  Refused before any device
 * call, as above and: NULL pointers, a source not 4-byte aligned, a payload that overlaps any source. */
int rrt_launch_exr_layers(void* d_payload, const rrt_exr_layers* layers, int width, int height, void* stream);

/* The same bytes on HOST memory (the sources' d_data are host pointers), from the source the kernels run; no device is touched */
int rrt_exr_layers_host(void* payload, const rrt_exr_layers* layers, int width, int height);

/* rrt_exr_header with the layers' channel list; cap 2048 always suffices */
int rrt_exr_layers_header(const rrt_exr_layers* layers, int width, int height, int fps_num, int fps_den, void* buf, size_t cap, size_t* len);

/* Why the last call on this thread returned RRT_ERR_INVALID_ARGUMENT, or the HIP runtime's message behind RRT_ERR_HIP ("" after a
 * call that succeeded) */
const char* rrt_exr_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RRT_EXR_H */
