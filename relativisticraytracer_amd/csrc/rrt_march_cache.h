/*
 * rrt_march_cache.h -- host bookkeeping of the march cache ("retained geodesics"): the launch key, the
 * per-device policy state machine and the capacity rule.  Plain C++: no HIP type, no device code (the kernels that fill and replay
 * the cache are in rrt_kernels.h, the object that owns the device memory in rrt_hip.hip), so that a host-only test can compile it
 * (tests/march_cache/policy_exerciser.cpp).
 *
 * What is cached: the output of pass 1 of the three-pass path (march_defer) for ONE launch key per device -- the pooled rows of
 * media sample points, the wave headers and the 28 B terminal state per ray.  Nothing in it depends on `time`, the sky, the
 * noise table or the effects that act after the march; passes 2 and 3 (eval_sample_rows, composite_and_shade) are re-run on it
 * every frame.
 * The fill's pass 2 rewrites every pooled row, in place, from the raw sample (position, vel.x, vel.z) into a SAMPLE RECORD
 * (csrc/rrt_device.h: SampleRecord; layout: kOutBlockEnv in rrt_kernels.h): the part of the sample's evaluation above the five
 * places where `time` enters -- cylindrical radius, height, azimuth, redshift factor, radius and the two density envelopes --
 * and clears the lanes whose envelopes are both 0 from the row's input mask.  A record depends on (rel_p, vel, spin, arith_mode)
 * only, all of them in the key or fixed by it; not on MEDIA, the tables, the sky or the effects.  Replays evaluate records.
 */
#ifndef RRT_MARCH_CACHE_H
#define RRT_MARCH_CACHE_H

#include <cstdint>
#include <cstring>

namespace rrt_mc {

/* Everything pass 1 and the row bookkeeping read, bit for bit.  Filled in ONE place (march_key() in rrt_hip.hip, next to the
 * tripwire on sizeof(FrameArgs)); compared with memcmp, so it is zeroed first and has no implicit padding. */
struct MarchKey {
    uint32_t cam[12];                  /* rrt_camera: pos, forward, right, up */
    int32_t width, height;
    int32_t n_local_rows, y_base, tile_rows, shard, n_shards;      /* RowMap (launches with an rrt_tile_map are not cached) */
    uint32_t spin;                     /* float bits; drag_c is a function of it */
    int32_t max_steps;
    int32_t nudge_ulps; uint32_t nudge_seed;
    int32_t arith_mode;
    int32_t volumetrics;
    int32_t use_lens; uint32_t distortion_amount;                  /* the one effect that moves a primary ray */
};
static_assert(sizeof(MarchKey) == 27 * 4, "MarchKey has no padding: it is compared with memcmp");

/* fields that cannot matter are cleared, so that they do not invalidate: the distortion amount with the lens off, the nudge
 * seed without a nudge */
inline void canonicalize(MarchKey& k) {
    if (k.use_lens == 0) k.distortion_amount = 0u;
    else k.use_lens = 1;
    if (k.nudge_ulps == 0) k.nudge_seed = 0u;
    k.volumetrics = k.volumetrics != 0 ? 1 : 0;
}
inline bool same_key(const MarchKey& a, const MarchKey& b) { return memcmp(&a, &b, sizeof(MarchKey)) == 0; }

enum Action {
    kToday = 0,      /* today's path; the key is remembered (first launch of a key, or a key that cannot be cached) */
    kFill = 1,       /* three passes, pass 1 writes the cache */
    kReplay = 2      /* passes 2 and 3 on the retained rows */
};
enum State { kNone = 0, kSeen, kPending, kRefill, kReady, kOff };
enum Why { kWhyNone = 0, kWhyBudget = 1, kWhyOverflow = 2, kWhyAlloc = 3 };

struct Stats {
    uint64_t fills, hits, drops, misses, uncacheable;
};

/* One key at a time.  A launch with another key costs nothing but the comparison: it runs today's code and only replaces the
 * remembered key.  The SECOND consecutive launch of a key fills, the third and later replay.  A fill the pool ran out under is
 * repeated once at a larger capacity (kRefill); if that overflows too, or no memory is to be had, the key is marked uncacheable
 * and stays on today's path until another key arrives (the object frees the memory of a key it has given up). */
struct Policy {
    MarchKey key;
    int state = kNone;
    bool grown = false;
    int why = kWhyNone;
    Stats st = {0, 0, 0, 0, 0};

    bool pending_for(const MarchKey& k) const { return state == kPending && same_key(k, key); }
    /* the fill of the current key has finished: did every ray's samples fit? */
    void fill_verified(bool complete) {
        if (state != kPending) return;
        if (complete) state = kReady;
        else if (!grown) state = kRefill;
        else { state = kOff; why = kWhyOverflow; }
    }
    /* the fill next() just asked for could not be enqueued (no memory inside the budget) */
    void fill_failed(int reason) {
        if (state == kPending) { --st.fills; ++st.uncacheable; }
        state = kOff; why = reason;
    }
    Action next(const MarchKey& k) {
        if (state == kNone || !same_key(k, key)) {
            if (state == kPending || state == kRefill || state == kReady) ++st.drops;
            key = k; state = kSeen; grown = false; why = kWhyNone;
            ++st.misses;
            return kToday;
        }
        switch (state) {
            case kSeen: state = kPending; ++st.fills; return kFill;
            case kRefill: grown = true; state = kPending; ++st.fills; return kFill;
            case kReady: ++st.hits; return kReplay;
            case kPending:           /* the caller verifies a pending fill before asking; without that: today's path */
            default: ++st.uncacheable; return kToday;
        }
    }
    /* forget the key (release, reconfigure) */
    void reset() {
        if (state == kPending || state == kRefill || state == kReady) ++st.drops;
        state = kNone; grown = false; why = kWhyNone;
    }
};

/* Capacity rule, in pool blocks.  The first fill of a key takes rays x kInitBytesPerRay of sample rows -- the 4K bench frame
 * pools 210 147 blocks = 2.18 GB for 8.29 M rays = 263 B per ray (profiles/r07_march_cache_ab.txt; rounds 1-3 measured 400,
 * LABNOTES.md "Pool appetite"), and 448 leaves a view with 1.7 times its media room in the first fill -- but never fewer than
 * kMinBlocks (a small frame from inside the disk needs ~10 KB per ray); a refill takes kGrowFactor times that.  Both are cut to
 * what the byte budget holds; fewer than kFloorBlocks: not cacheable. */
constexpr uint64_t kInitBytesPerRay = 448;
constexpr uint64_t kMinBlocks = 16384, kFloorBlocks = 1024, kGrowFactor = 8;
inline uint64_t wanted_blocks(uint64_t rays, uint64_t in_block_bytes, bool grown) {
    uint64_t b = rays * kInitBytesPerRay / in_block_bytes;
    if (b < kMinBlocks) b = kMinBlocks;
    if (grown) b *= kGrowFactor;
    if (b > 0x0fffffffull) b = 0x0fffffffull;
    return b;
}
/* blocks of `block_bytes` (rows in + evaluated planes out) that fit `budget` next to `fixed` bytes of bookkeeping; 0: none */
inline uint64_t blocks_in_budget(uint64_t wanted, uint64_t budget, uint64_t fixed, uint64_t block_bytes) {
    if (budget <= fixed) return 0;
    const uint64_t fit = (budget - fixed) / block_bytes;
    const uint64_t b = wanted < fit ? wanted : fit;
    return b < kFloorBlocks ? 0 : b;
}

}  // namespace rrt_mc

#endif
