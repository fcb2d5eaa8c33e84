/*
 * rrt_deflate_core.h -- the definition of include/rrt_deflate.h as functions the host and the device share (RRT_FN, as
 * rrt_png_core.h): plain C++ that g++ can include.  rrt_deflate.hip's deflate_segments kernel, rrt_deflate_host and
 * tests/deflate/deflate_exerciser.cpp run this very source.
 *
 * A segment is coded by RRT_DEFLATE_THREADS threads over one DeflateWork (LDS on the device) in PHASES: a phase is a function of
 * (work, tid) that every thread runs, and a barrier stands between two phases.  dfl_fragment lists the phases once, for an executor
 * that says what "every thread" means: the kernel's runs the phase on its own thread and then __syncthreads; the host's runs it for
 * tid = 0 ... 255 in turn.  So the host entry point is the kernel's program, thread for thread, and what two threads of a phase
 * share they share through DFL_ADD / DFL_OR alone (LDS atomics on the device).
 *
 * The split: thread c owns CHUNK c, the segment's bytes 128 c ... 128 c + 127.  A token belongs to the chunk it starts in.  Which
 * tokens start in a chunk follows from step 2's closed form once the chunk knows where the run that reaches into it began (a max-scan
 * over the chunks' last run starts) and where the run that leaves it ends (a min-scan, from the right, over their first run starts).
 */
#ifndef RRT_DEFLATE_CORE_H
#define RRT_DEFLATE_CORE_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
#endif

#include "../../include/rrt_deflate.h"
#include "rrt_math.h"     /* RRT_FN */

#if defined(__HIPCC__)
#define DFL_MFN __host__ __device__ __forceinline__
#else
#define DFL_MFN inline __attribute__((always_inline))
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define DFL_ADD(p, v) atomicAdd((p), (v))
#define DFL_OR(p, v) atomicOr((p), (v))
#else
#define DFL_ADD(p, v) (*(p) += (v))
#define DFL_OR(p, v) (*(p) |= (v))
#endif

constexpr int kDflThreads = RRT_DEFLATE_THREADS;
constexpr int kDflChunk = RRT_DEFLATE_CHUNK_BYTES;
constexpr uint32_t kDflSegment = RRT_DEFLATE_SEGMENT_BYTES;
constexpr int kDflEob = 256;
constexpr int kDflClSymbols = 19;
constexpr int kDflSeqMax = 320;                              /* entries of a run-length coded length sequence: <= 288 */
constexpr int kDflBitWords = (int)(kDflSegment + 64u) / 4;   /* the fragment is built here: at most m + 10 bytes, rounded up to 16 */
constexpr uint32_t kDflSlotPad = 48u;                        /* scratch: a fragment's slot is 16-byte aligned and holds m + 10 rounded up to 16 */
static_assert(kDflThreads * kDflChunk == (int)kDflSegment, "a thread per chunk");

struct alignas(16) DflQuad { uint32_t x, y, z, w; };

/* lengths(counts, limit) over at most N symbols: step 4's working set, and step 5's codes */
template <int N>
struct DeflateHuff {
    uint32_t cnt[N];             /* the counts; halved in place */
    uint32_t wt[2 * N];          /* node weights: the sorted leaves 0 ... used - 1, then the internal nodes in order of creation */
    uint16_t order[N];           /* the symbol of sorted leaf r */
    uint16_t parent[2 * N];
    uint16_t depth[2 * N];
    uint16_t code[N];            /* bit-reversed */
    uint8_t len[N];
    uint32_t per_len[16], next[16];
    int32_t n, limit, used, redo, halvings;
};

struct DeflateWork {
    DflQuad in[kDflSegment / 16 + 2];        /* the segment, shifted by `shift` bytes: 16-byte words of the input land on 16-byte words */
    uint32_t bits[kDflBitWords];             /* the fragment */
    DeflateHuff<RRT_DEFLATE_MAX_SYMBOLS> ll;
    DeflateHuff<32> cl;
    uint32_t sa[2][kDflThreads], sb[2][kDflThreads];      /* two scans at a time, ping-pong */
    uint32_t run_in[kDflThreads], run_next[kDflThreads];    /* the start of the run that reaches into a chunk; the first run start behind it */
    uint8_t seq_sym[kDflSeqMax], seq_extra[kDflSeqMax];   /* step 6's run-length coded sequence */
    uint32_t m, shift, final;
    int32_t n_seq, nll, ncl;
    uint32_t header_bits, body_bits, stored, frag_len;
};
static_assert(sizeof(DeflateWork) <= 80 * 1024, "two workgroups per CU: 160 KiB of LDS");

/* what a workgroup is told about its segment */
struct DeflateSeg {
    const uint8_t* src;      /* the whole input, and its size: the 16-byte loads stay inside it */
    uint64_t n;
    uint64_t off;            /* the segment's first byte */
    uint32_t m;
    uint32_t final;          /* step 9's F */
};

/* The cut, computed once on the host and passed by value */
struct DeflatePlan {
    uint64_t n, stream_bytes;
    uint64_t n_streams, per_stream;          /* segments of every stream but the last */
    uint64_t last_len, last_segs, n_segments;
    uint64_t table_bytes;                    /* scratch: lens[n_segments], offs[n_segments] (uint32 each), rounded up to 16 */
    int32_t finish;
};

RRT_FN DeflateSeg dfl_segment(const DeflatePlan& p, const void* src, uint64_t g) {
    uint64_t j = g / p.per_stream;
    if (j > p.n_streams - 1) j = p.n_streams - 1;
    const uint64_t i = g - j * p.per_stream;
    const uint64_t slen = j < p.n_streams - 1 ? p.stream_bytes : p.last_len;
    const uint64_t rest = slen - i * kDflSegment;
    DeflateSeg s;
    s.src = static_cast<const uint8_t*>(src);
    s.n = p.n;
    s.off = j * p.stream_bytes + i * kDflSegment;
    s.m = (uint32_t)(rest < kDflSegment ? rest : kDflSegment);
    s.final = (p.finish && g == p.n_segments - 1) ? 1u : 0u;
    return s;
}

RRT_FN uint64_t dfl_slot_offset(const DeflatePlan& p, uint64_t g, uint64_t off) { return p.table_bytes + ((off + 15u) & ~(uint64_t)15u) + kDflSlotPad * g; }

RRT_FN const uint8_t* dfl_bytes(const DeflateWork& w) { return reinterpret_cast<const uint8_t*>(w.in) + w.shift; }

/* ---- the tokens of a chunk ---------------------------------------------------------------------------------------------------- */

/* RFC 1951's length code of a match of L = 3 ... 258 bytes */
RRT_FN void dfl_length_code(uint32_t L, uint32_t& sym, uint32_t& extra_bits, uint32_t& extra) {
    const uint32_t x = L - 3u;
    if (L == 258u) { sym = 285u; extra_bits = 0u; extra = 0u; return; }
    if (x < 8u) { sym = 257u + x; extra_bits = 0u; extra = 0u; return; }
    const uint32_t hb = 31u - (uint32_t)__builtin_clz(x);       /* the highest set bit: 3 ... 7 */
    extra_bits = hb - 2u;
    sym = 261u + 4u * extra_bits + ((x - (1u << hb)) >> extra_bits);
    extra = x & ((1u << extra_bits) - 1u);
}

/* f.literal(byte) / f.match(L) for every token that starts in chunk c, in order (step 2's closed form) */
template <class F>
RRT_FN void dfl_walk(const DeflateWork& w, int c, F& f) {
    const int m = (int)w.m, lo = c * kDflChunk;
    if (lo >= m) return;
    const int hi = lo + kDflChunk < m ? lo + kDflChunk : m;
    const uint8_t* b = dfl_bytes(w);
    int p = lo;
    while (p < hi) {
        const bool start = p == 0 || b[p] != b[p - 1];
        const int s = start ? p : (int)w.run_in[c];      /* only the chunk's first byte can lie inside a run */
        int q = p + 1;
        while (q < hi && b[q] == b[p]) ++q;
        const int e = (q == hi && hi < m) ? (int)w.run_next[c] : q;       /* the run's end: the next run start */
        const int end = e < hi ? e : hi;
        const int tail = e - s - 1, full = tail / 258, rem = tail - 258 * full, jf = 258 * full;
        if (start) f.literal(b[p]);
        /* the run's tail, bytes s + 1 ... e - 1, by index j: matches of 258 at j = 0, 258, ... < jf, then the remainder at jf */
        int j = (start ? p + 1 : p) - (s + 1);
        const int j_end = end - (s + 1);
        if (j < jf) {
            j = ((j + 257) / 258) * 258;
            for (; j < jf && j < j_end; j += 258) f.match(258u);
        }
        if (j < j_end) {
            if (rem >= 3) {
                if (j == jf) f.match((uint32_t)rem);
            } else {
                for (; j < j_end; ++j) f.literal(b[p]);
            }
        }
        p = end;
    }
}

struct DflCount {
    DeflateWork& w;
    DFL_MFN void literal(uint32_t v) { DFL_ADD(&w.ll.cnt[v], 1u); }
    DFL_MFN void match(uint32_t L) {
        uint32_t sym, eb, ex;
        dfl_length_code(L, sym, eb, ex);
        DFL_ADD(&w.ll.cnt[sym], 1u);
    }
};

struct DflMeasure {
    const DeflateWork& w;
    uint32_t bits;
    DFL_MFN void literal(uint32_t v) { bits += w.ll.len[v]; }
    DFL_MFN void match(uint32_t L) {
        uint32_t sym, eb, ex;
        dfl_length_code(L, sym, eb, ex);
        bits += w.ll.len[sym] + eb + 1u;
    }
};

/* bits appended from bit `pos` on: whole words that lie inside the thread's own range are stored, the two it may share are OR-ed */
struct DflEmit {
    DeflateWork& w;
    uint64_t acc;
    uint32_t nacc, word;
    bool shared;
    DFL_MFN void begin(uint32_t pos) { acc = 0; nacc = pos & 31u; word = pos >> 5; shared = nacc != 0u; }
    DFL_MFN void put(uint32_t v, uint32_t nb) {          /* nb <= 21 */
        acc |= (uint64_t)v << nacc;
        nacc += nb;
        if (nacc >= 32u) {
            if (shared) DFL_OR(&w.bits[word], (uint32_t)acc);
            else w.bits[word] = (uint32_t)acc;
            shared = false;
            acc >>= 32;
            nacc -= 32u;
            ++word;
        }
    }
    DFL_MFN void end() { if (nacc != 0u) DFL_OR(&w.bits[word], (uint32_t)acc); }
    DFL_MFN void literal(uint32_t v) { put(w.ll.code[v], w.ll.len[v]); }
    DFL_MFN void match(uint32_t L) {
        uint32_t sym, eb, ex;
        dfl_length_code(L, sym, eb, ex);
        put((uint32_t)w.ll.code[sym] | (ex << w.ll.len[sym]), w.ll.len[sym] + eb + 1u);      /* code, extra bits, distance 1: the bit 0 */
    }
};

/* ---- the phases ----------------------------------------------------------------------------------------------------------------- */

/* the segment into LDS, 16 bytes at a time; a 16-byte word that the input's ends cut is loaded byte by byte.  Zeros what is summed. */
RRT_FN void dfl_stage(DeflateWork& w, const DeflateSeg& s, int tid) {
    const uintptr_t first = (uintptr_t)s.src + (uintptr_t)s.off, lo = (uintptr_t)s.src, hi = (uintptr_t)s.src + (uintptr_t)s.n;
    const uint32_t shift = (uint32_t)(first & 15u);
    const uintptr_t base = first - shift;
    const uint32_t nq = (shift + s.m + 15u) / 16u;
    for (uint32_t q = (uint32_t)tid; q < nq; q += (uint32_t)kDflThreads) {
        const uintptr_t a = base + 16u * (uintptr_t)q;
        if (a >= lo && a + 16u <= hi) {
            w.in[q] = *reinterpret_cast<const DflQuad*>(a);
        } else {
            uint8_t* dst = reinterpret_cast<uint8_t*>(&w.in[q]);
            for (uint32_t k = 0; k < 16u; ++k) dst[k] = (a + k >= lo && a + k < hi) ? *reinterpret_cast<const uint8_t*>(a + k) : (uint8_t)0;
        }
    }
    for (int i = tid; i < RRT_DEFLATE_MAX_SYMBOLS; i += kDflThreads) w.ll.cnt[i] = 0u;
    if (tid < 32) w.cl.cnt[tid] = 0u;
    const uint32_t nw = ((s.m + 10u + 15u) / 16u) * 4u;
    for (uint32_t i = (uint32_t)tid; i < nw; i += (uint32_t)kDflThreads) w.bits[i] = 0u;
    if (tid == 0) {
        w.m = s.m;
        w.shift = shift;
        w.final = s.final;
        w.ll.n = RRT_DEFLATE_LL_SYMBOLS;
        w.ll.limit = 15;
        w.cl.n = kDflClSymbols;
        w.cl.limit = 7;
    }
}

/* chunk c's last run start + 1 (0: none) and its first run start (m: none), for the two scans */
RRT_FN void dfl_run_starts(DeflateWork& w, int c) {
    const int m = (int)w.m, lo = c * kDflChunk;
    const int hi = lo + kDflChunk < m ? lo + kDflChunk : m;
    const uint8_t* b = dfl_bytes(w);
    uint32_t first = (uint32_t)m, last = 0u;
    for (int p = lo; p < hi; ++p) {
        if (p == 0 || b[p] != b[p - 1]) {
            if (first == (uint32_t)m) first = (uint32_t)p;
            last = (uint32_t)p + 1u;
        }
    }
    w.sa[0][c] = last;
    w.sb[0][kDflThreads - 1 - c] = first;
}

/* one step of two inclusive scans over the 256 chunks, from buffer `from` into the other: sa a maximum (sum = false) or a sum,
 * sb a minimum.  Eight steps, offsets 1 ... 128, leave the results in buffer 0. */
RRT_FN void dfl_scan_step(DeflateWork& w, int tid, int off, int from, bool sum) {
    uint32_t a = w.sa[from][tid], b = w.sb[from][tid];
    if (tid >= off) {
        const uint32_t a2 = w.sa[from][tid - off], b2 = w.sb[from][tid - off];
        a = sum ? a + a2 : (a2 > a ? a2 : a);
        b = b2 < b ? b2 : b;
    }
    w.sa[from ^ 1][tid] = a;
    w.sb[from ^ 1][tid] = b;
}

/* After the scans sa[0][c] - 1 is the last run start at or before chunk c's end, sb[0][255 - c] the first one in chunk c or behind it */
RRT_FN void dfl_count(DeflateWork& w, int tid) {
    w.run_in[tid] = tid > 0 ? w.sa[0][tid - 1] - 1u : 0u;
    w.run_next[tid] = tid < kDflThreads - 1 ? w.sb[0][kDflThreads - 2 - tid] : w.m;
    DflCount f = {w};
    dfl_walk(w, tid, f);
    if (tid == 0) DFL_ADD(&w.ll.cnt[kDflEob], 1u);
}

/* step 4, the start: how many symbols are used */
template <int N>
RRT_FN void dfl_huff_begin(DeflateHuff<N>& h, int tid) {
    if (tid == 0) { h.used = 0; h.halvings = 0; h.redo = 0; }
}
template <int N>
RRT_FN void dfl_huff_used(DeflateHuff<N>& h, int tid) {
    for (int i = tid; i < h.n; i += kDflThreads)
        if (h.cnt[i] != 0u) DFL_ADD(&h.used, 1);
}
template <int N>
RRT_FN void dfl_huff_single(DeflateHuff<N>& h, int tid) {
    if (tid == 0 && h.used == 1) {
        h.cnt[h.cnt[0] != 0u ? 1 : 0] = 1u;          /* the lowest-numbered unused symbol */
        h.used = 2;
    }
}
/* the leaves sorted by (count, symbol): every used symbol finds its own rank */
template <int N>
RRT_FN void dfl_huff_rank(DeflateHuff<N>& h, int tid) {
    for (int i = tid; i < h.n; i += kDflThreads) {
        h.len[i] = 0;
        const uint32_t ci = h.cnt[i];
        if (ci == 0u) continue;
        int rank = 0;
        for (int j = 0; j < h.n; ++j) {
            const uint32_t cj = h.cnt[j];
            rank += (cj != 0u && (cj < ci || (cj == ci && j < i))) ? 1 : 0;
        }
        h.order[rank] = (uint16_t)i;
        h.wt[rank] = ci;
    }
    if (tid < 16) h.per_len[tid] = 0u;
}
/* the two-queue merge and the depths, on one thread: at most N - 1 steps */
template <int N>
RRT_FN void dfl_huff_merge(DeflateHuff<N>& h, int tid) {
    if (tid != 0) return;
    const int k = h.used;
    h.redo = 0;
    if (k < 2) return;
    int leaf = 0, inner = k, next = k;
    while (next < 2 * k - 1) {
        uint32_t sum = 0u;
        for (int t = 0; t < 2; ++t) {
            int v;
            if (leaf < k && (inner >= next || h.wt[leaf] <= h.wt[inner])) v = leaf++;        /* a tie goes to the leaf */
            else v = inner++;
            sum += h.wt[v];
            h.parent[v] = (uint16_t)next;
        }
        h.wt[next++] = sum;
    }
    h.depth[2 * k - 2] = 0;
    int deepest = 0;
    for (int v = 2 * k - 3; v >= 0; --v) {
        const int d = h.depth[h.parent[v]] + 1;
        h.depth[v] = (uint16_t)d;
        if (v < k && d > deepest) deepest = d;
    }
    if (deepest > h.limit) {
        h.redo = 1;
        ++h.halvings;
    }
}
/* too deep: halve and merge again; otherwise a leaf's length is its depth */
template <int N>
RRT_FN void dfl_huff_settle(DeflateHuff<N>& h, int tid) {
    if (h.redo) {
        for (int i = tid; i < h.n; i += kDflThreads)
            if (h.cnt[i] != 0u) h.cnt[i] = (h.cnt[i] + 1u) >> 1;
    } else {
        for (int r = tid; r < h.used; r += kDflThreads) {
            h.len[h.order[r]] = (uint8_t)h.depth[r];
            DFL_ADD(&h.per_len[h.depth[r]], 1u);
        }
    }
}
/* step 5 */
template <int N>
RRT_FN void dfl_huff_first_codes(DeflateHuff<N>& h, int tid) {
    if (tid != 0) return;
    uint32_t code = 0u;
    h.per_len[0] = 0u;
    h.next[0] = 0u;
    for (int bits = 1; bits <= 15; ++bits) {
        code = (code + h.per_len[bits - 1]) << 1;
        h.next[bits] = code;
    }
}
template <int N>
RRT_FN void dfl_huff_codes(DeflateHuff<N>& h, int tid) {
    for (int i = tid; i < h.n; i += kDflThreads) {
        const uint32_t l = h.len[i];
        uint32_t c = 0u;
        if (l != 0u) {
            c = h.next[l];
            for (int j = 0; j < i; ++j) c += h.len[j] == l ? 1u : 0u;
        }
        uint32_t r = 0u;
        for (uint32_t k = 0; k < l; ++k) r |= ((c >> k) & 1u) << (l - 1u - k);
        h.code[i] = (uint16_t)r;
    }
}

template <class X, int N>
RRT_FN void dfl_lengths(X& x, DeflateHuff<N>& h) {
    x.run([&](int tid) { dfl_huff_begin(h, tid); });
    x.run([&](int tid) { dfl_huff_used(h, tid); });
    x.run([&](int tid) { dfl_huff_single(h, tid); });
    do {
        x.run([&](int tid) { dfl_huff_rank(h, tid); });
        x.run([&](int tid) { dfl_huff_merge(h, tid); });
        x.run([&](int tid) { dfl_huff_settle(h, tid); });
    } while (h.redo);
}

template <class X, int N>
RRT_FN void dfl_codes(X& x, DeflateHuff<N>& h) {
    x.run([&](int tid) { dfl_huff_first_codes(h, tid); });
    x.run([&](int tid) { dfl_huff_codes(h, tid); });
}

/* step 6, first half: the literal/length lengths and the two distance lengths as one run-length coded sequence, and its counts */
RRT_FN void dfl_sequence(DeflateWork& w, int tid) {
    if (tid != 0) return;
    int nll = RRT_DEFLATE_LL_SYMBOLS;
    while (nll > 257 && w.ll.len[nll - 1] == 0) --nll;
    w.nll = nll;
    const int total = nll + 2;
    int n = 0;
    auto emit = [&](uint32_t sym, uint32_t extra) {
        w.seq_sym[n] = (uint8_t)sym;
        w.seq_extra[n] = (uint8_t)extra;
        ++n;
        ++w.cl.cnt[sym];
    };
    int i = 0;
    while (i < total) {
        const uint32_t v = i < nll ? w.ll.len[i] : 1u;
        int run = 1;
        while (i + run < total && (i + run < nll ? w.ll.len[i + run] : 1u) == v) ++run;
        i += run;
        if (v == 0u) {
            while (run >= 11) {
                const int t = run < 138 ? run : 138;
                emit(18u, (uint32_t)(t - 11));
                run -= t;
            }
            if (run >= 3) {
                emit(17u, (uint32_t)(run - 3));
                run = 0;
            }
            for (; run > 0; --run) emit(0u, 0u);
        } else {
            emit(v, 0u);
            --run;
            while (run >= 3) {
                const int t = run < 6 ? run : 6;
                emit(16u, (uint32_t)(t - 3));
                run -= t;
            }
            for (; run > 0; --run) emit(v, 0u);
        }
    }
    w.n_seq = n;
}

RRT_FN uint32_t dfl_seq_extra_bits(uint32_t sym) { return sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u; }

RRT_FN int dfl_cl_order(int i) {
    const uint8_t order[kDflClSymbols] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}

/* step 6, second half: the header's size */
RRT_FN void dfl_header_size(DeflateWork& w, int tid) {
    if (tid != 0) return;
    int ncl = kDflClSymbols;
    while (ncl > 4 && w.cl.len[dfl_cl_order(ncl - 1)] == 0) --ncl;
    w.ncl = ncl;
    uint32_t bits = 3u + 5u + 5u + 4u + 3u * (uint32_t)ncl;
    for (int i = 0; i < w.n_seq; ++i) bits += w.cl.len[w.seq_sym[i]] + dfl_seq_extra_bits(w.seq_sym[i]);
    w.header_bits = bits;
}

/* step 7's size, chunk by chunk, for the sum scan */
RRT_FN void dfl_measure(DeflateWork& w, int tid) {
    DflMeasure f = {w, 0u};
    dfl_walk(w, tid, f);
    w.sa[0][tid] = f.bits;
    w.sb[0][tid] = 0u;
}

/* step 8 */
RRT_FN void dfl_decide(DeflateWork& w, int tid) {
    if (tid != 0) return;
    w.body_bits = w.sa[0][kDflThreads - 1] + w.ll.len[kDflEob];
    const uint32_t d = (w.header_bits + w.body_bits + 3u + 7u) / 8u + 4u;
    w.stored = d >= w.m + 10u ? 1u : 0u;
    w.frag_len = w.stored ? w.m + 10u : d;
}

RRT_FN void dfl_or_bits(DeflateWork& w, uint32_t& pos, uint32_t v, uint32_t nb) {
    const uint64_t x = (uint64_t)v << (pos & 31u);
    DFL_OR(&w.bits[pos >> 5], (uint32_t)x);
    if ((uint32_t)(x >> 32) != 0u) DFL_OR(&w.bits[(pos >> 5) + 1u], (uint32_t)(x >> 32));
    pos += nb;
}

/* steps 6-9 into w.bits */
RRT_FN void dfl_emit(DeflateWork& w, int tid) {
    uint8_t* out = reinterpret_cast<uint8_t*>(w.bits);
    if (w.stored) {
        const uint8_t* b = dfl_bytes(w);
        for (uint32_t i = (uint32_t)tid; i < w.m; i += (uint32_t)kDflThreads) out[5u + i] = b[i];
        if (tid == 0) {
            out[0] = 0;                              /* BFINAL 0, BTYPE 00, pad */
            out[1] = (uint8_t)(w.m & 255u);
            out[2] = (uint8_t)(w.m >> 8);
            out[3] = (uint8_t)(~w.m & 255u);
            out[4] = (uint8_t)((~w.m >> 8) & 255u);
            uint8_t* t = out + 5u + w.m;
            t[0] = (uint8_t)w.final; t[1] = 0; t[2] = 0; t[3] = 0xff; t[4] = 0xff;
        }
        return;
    }
    DflEmit f = {w, 0, 0u, 0u, false};
    f.begin(w.header_bits + (tid > 0 ? w.sa[0][tid - 1] : 0u));
    dfl_walk(w, tid, f);
    f.end();
    if (tid != 0) return;
    uint32_t pos = 0u;
    dfl_or_bits(w, pos, 0u | (2u << 1), 3u);                  /* BFINAL 0, BTYPE 2 */
    dfl_or_bits(w, pos, (uint32_t)(w.nll - 257), 5u);
    dfl_or_bits(w, pos, 1u, 5u);                              /* HDIST: two distance codes */
    dfl_or_bits(w, pos, (uint32_t)(w.ncl - 4), 4u);
    for (int i = 0; i < w.ncl; ++i) dfl_or_bits(w, pos, w.cl.len[dfl_cl_order(i)], 3u);
    for (int i = 0; i < w.n_seq; ++i) {
        const uint32_t sym = w.seq_sym[i];
        dfl_or_bits(w, pos, w.cl.code[sym], w.cl.len[sym]);
        dfl_or_bits(w, pos, w.seq_extra[i], dfl_seq_extra_bits(sym));
    }
    pos = w.header_bits + w.body_bits - w.ll.len[kDflEob];
    dfl_or_bits(w, pos, w.ll.code[kDflEob], w.ll.len[kDflEob]);
    dfl_or_bits(w, pos, w.final, 3u);                         /* step 9: F, BTYPE 00 */
    pos = (pos + 7u) & ~7u;
    dfl_or_bits(w, pos, 0u, 16u);
    dfl_or_bits(w, pos, 0xffffu, 16u);
}

/* an empty segment: step 9 alone */
RRT_FN void dfl_empty(DeflateWork& w, const DeflateSeg& s, int tid) {
    if (tid != 0) return;
    w.m = 0u;
    w.final = s.final;
    w.stored = 0u;
    w.frag_len = 5u;
    w.bits[0] = s.final | 0xff000000u;          /* F, 00, 00, FF */
    w.bits[1] = 0x000000ffu;                    /* FF */
    w.bits[2] = w.bits[3] = 0u;
}

/* The fragment of segment s into w.bits, w.frag_len bytes of it.  X::run(f): f(tid) for every thread, then a barrier. */
template <class X>
RRT_FN void dfl_fragment(X& x, DeflateWork& w, const DeflateSeg& s) {
    if (s.m == 0u) {
        x.run([&](int tid) { dfl_empty(w, s, tid); });
        return;
    }
    x.run([&](int tid) { dfl_stage(w, s, tid); });
    x.run([&](int tid) { dfl_run_starts(w, tid); });
    for (int off = 1, from = 0; off < kDflThreads; off <<= 1, from ^= 1) x.run([&](int tid) { dfl_scan_step(w, tid, off, from, false); });
    x.run([&](int tid) { dfl_count(w, tid); });
    dfl_lengths(x, w.ll);
    dfl_codes(x, w.ll);
    x.run([&](int tid) { dfl_sequence(w, tid); });
    dfl_lengths(x, w.cl);
    dfl_codes(x, w.cl);
    x.run([&](int tid) { dfl_header_size(w, tid); });
    x.run([&](int tid) { dfl_measure(w, tid); });
    for (int off = 1, from = 0; off < kDflThreads; off <<= 1, from ^= 1) x.run([&](int tid) { dfl_scan_step(w, tid, off, from, true); });
    x.run([&](int tid) { dfl_decide(w, tid); });
    x.run([&](int tid) { dfl_emit(w, tid); });
}

/* ---- host only: the plan, the refusals, the geometry, the host entry points ---------------------------------------------------------------------------------------------- */

static thread_local char g_dfl_err[256] = "";

static inline int dfl_refuse(const char* what) {
    snprintf(g_dfl_err, sizeof(g_dfl_err), "%s", what);
    return RRT_ERR_INVALID_ARGUMENT;
}

static inline uint64_t dfl_out_bound(const DeflatePlan& p) { return p.n == 0 ? 5u : p.n + 10u * p.n_segments; }
static inline uint64_t dfl_scratch_bytes(const DeflatePlan& p) { return p.table_bytes + ((p.n + 15u) & ~(uint64_t)15u) + kDflSlotPad * p.n_segments + 64u; }

static inline int dfl_plan(size_t n, size_t stream_bytes, int finish, DeflatePlan& p) {
    g_dfl_err[0] = 0;
    if ((uint64_t)n >= ((uint64_t)1 << 32)) return dfl_refuse("n is 2^32 or more");
    if (stream_bytes < 1) return dfl_refuse("stream_bytes >= 1");
    if (finish != 0 && finish != 1) return dfl_refuse("finish: 0 | 1");
    p.n = n;
    p.stream_bytes = stream_bytes;
    p.n_streams = n == 0 ? 1u : ((uint64_t)n + stream_bytes - 1u) / stream_bytes;
    const uint64_t full = stream_bytes < n ? stream_bytes : n;          /* a stream that is not the last holds stream_bytes <= n bytes */
    p.per_stream = full == 0 ? 1u : (full + kDflSegment - 1u) / kDflSegment;
    p.last_len = n - (p.n_streams - 1u) * stream_bytes;
    p.last_segs = p.last_len == 0 ? 1u : (p.last_len + kDflSegment - 1u) / kDflSegment;
    p.n_segments = (p.n_streams - 1u) * p.per_stream + p.last_segs;
    p.table_bytes = (8u * p.n_segments + 15u) & ~(uint64_t)15u;
    p.finish = finish;
    if (dfl_out_bound(p) >= ((uint64_t)1 << 32)) return dfl_refuse("an out_bound of 2^32 bytes or more");
    return RRT_OK;
}

static inline bool dfl_overlap(uintptr_t a, uint64_t a_bytes, uintptr_t b, uint64_t b_bytes) { return a < b + b_bytes && b < a + a_bytes; }

/* out[12] of rrt_deflate_launch_geometry */
static inline void dfl_geometry(const DeflatePlan& p, size_t address_bits, int32_t out[12]) {
    out[0] = kDflThreads; out[1] = (int32_t)p.n_segments; out[2] = (int32_t)sizeof(DeflateWork);
    out[3] = kDflThreads; out[4] = 1; out[5] = (int32_t)(kDflThreads * sizeof(uint32_t));
    out[6] = kDflThreads; out[7] = (int32_t)p.n_segments; out[8] = 0;
    /* the 16-byte words of the address space that lie wholly inside the input are loaded whole (dfl_stage); what its ends cut, byte by byte */
    const uint64_t a = address_bits & 15u, e = a + p.n;
    const uint64_t first_whole = (a + 15u) & ~(uint64_t)15u, last_whole = e & ~(uint64_t)15u;
    const bool any = last_whole > first_whole;
    out[9] = (int32_t)(any ? first_whole - a : p.n);
    out[10] = (int32_t)(any ? e - last_whole : 0u);
    out[11] = (int32_t)(any ? (last_whole - first_whole) / 16u : 0u);
}

struct DflHostThreads {
    template <class F>
    void run(F f) {
        for (int tid = 0; tid < kDflThreads; ++tid) f(tid);
    }
};

static inline int dfl_code_lengths(const uint32_t* counts, int n_symbols, int limit, uint8_t* lengths_out, int32_t* halvings) {
    g_dfl_err[0] = 0;
    if (!counts || !lengths_out) return dfl_refuse("counts or lengths_out is NULL");
    if (n_symbols < 2 || n_symbols > RRT_DEFLATE_MAX_SYMBOLS) return dfl_refuse("n_symbols: 2 ... RRT_DEFLATE_MAX_SYMBOLS");
    if (limit < 1 || limit > 15 || (1 << limit) < n_symbols) return dfl_refuse("limit: 1 ... 15, and 2^limit >= n_symbols");
    uint64_t sum = 0;
    for (int i = 0; i < n_symbols; ++i) sum += counts[i];
    if (sum >= ((uint64_t)1 << 32)) return dfl_refuse("the counts' sum is 2^32 or more");
    std::vector<DeflateHuff<RRT_DEFLATE_MAX_SYMBOLS>> work(1);
    DeflateHuff<RRT_DEFLATE_MAX_SYMBOLS>& h = work[0];
    memset(&h, 0, sizeof(h));
    for (int i = 0; i < n_symbols; ++i) h.cnt[i] = counts[i];
    h.n = n_symbols;
    h.limit = limit;
    DflHostThreads x;
    dfl_lengths(x, h);
    for (int i = 0; i < n_symbols; ++i) lengths_out[i] = h.len[i];
    if (halvings) *halvings = h.halvings;
    return RRT_OK;
}

static inline int dfl_host(void* out, uint32_t* stream_sizes, const void* src, size_t n, size_t stream_bytes, int finish, size_t* total) {
    DeflatePlan p;
    const int rc = dfl_plan(n, stream_bytes, finish, p);
    if (rc != RRT_OK) return rc;
    if (!out || !stream_sizes || (!src && n != 0)) return dfl_refuse("out, stream_sizes or src is NULL");
    const uintptr_t o = (uintptr_t)out, tab = (uintptr_t)stream_sizes, in = (uintptr_t)src;
    if ((tab & 3u) != 0) return dfl_refuse("stream_sizes is not 4-byte aligned");
    const uint64_t out_b = dfl_out_bound(p), tab_b = 4u * p.n_streams;
    if (n != 0 && (dfl_overlap(o, out_b, in, n) || dfl_overlap(tab, tab_b, in, n))) return dfl_refuse("an output overlaps the input");
    if (dfl_overlap(o, out_b, tab, tab_b)) return dfl_refuse("the outputs overlap each other");
    std::vector<DeflateWork> work(1);
    DflHostThreads x;
    uint8_t* dst = static_cast<uint8_t*>(out);
    uint64_t at = 0;
    for (uint64_t j = 0; j < p.n_streams; ++j) stream_sizes[j] = 0u;
    for (uint64_t g = 0; g < p.n_segments; ++g) {
        const DeflateSeg s = dfl_segment(p, src, g);
        dfl_fragment(x, work[0], s);
        memcpy(dst + at, work[0].bits, work[0].frag_len);
        at += work[0].frag_len;
        const uint64_t j = g / p.per_stream < p.n_streams - 1u ? g / p.per_stream : p.n_streams - 1u;
        stream_sizes[j] += work[0].frag_len;
    }
    if (total) *total = (size_t)at;
    return RRT_OK;
}

#endif
