/*
 * rrt_test_records.h -- test hooks of the march cache's sample records (csrc/rrt_device.h: SampleRecord): NOT part of the product.
 *
 * librrt_hip_test.so only (the sources built with -DRRT_TEST_HOOKS).  The function exports of that library are exactly those of
 * the product plus what include/rrt_test.h declares, and stay so: these two hooks are reached through ONE exported object, a
 * table of function pointers, `rrt_test_records`.  A caller checks `struct_size` before it uses an entry.
 */
#ifndef RRT_TEST_RECORDS_H
#define RRT_TEST_RECORDS_H

#include "rrt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rrt_test_records_table {
    uint32_t struct_size;
    uint32_t reserved;
    /* The sample records against today's evaluation of a pooled sample, through the PRODUCTION pass 2 (eval_sample_rows) on pool
     * rows the hook lays out: element i is lane i % 64 of row i / 64.  d_p / d_vel: n sample points and ray velocities (x, y, z
     * each); times: n_times >= 1 values on the HOST.  For every time t:
     *   d_has_raw / d_out_raw [t * n + i]   the non-KEEP instance on the raw rows (today's evaluation)
     *   d_has_rec / d_out_rec [t * n + i]   the KEEP instance: t = 0 as the march cache's FILL (raw row -> record in place, input
     *                                       masks pruned, the frame from the derived values), t >= 1 as REPLAYS of those records
     * has: 1 where raymarcher.cu:71 takes the sample; out: (ex, ey, ez, transmittance), (0, 0, 0, 1) where it does not.
     * d_records: n x 7 floats, what the fill left (rc, y, azimuth, shift_g, r, env_acc, env_dust); d_kept: 1 where the lane is
     * still in its row's input mask.  table: a noise table or 0; a time outside its window runs the arithmetic instance, as a
     * launch does.  arith_mode: RRT_ARITH_*.  Allocates its pool, synchronises the stream and frees it. */
    int (*sample_records)(int n, const float* d_p, const float* d_vel, float spin, int arith_mode, int table, int n_times,
                          const float* times, int32_t* d_has_raw, float* d_out_raw, int32_t* d_has_rec, float* d_out_rec,
                          float* d_records, int32_t* d_kept, void* stream);
    /* the last fill of `device`'s march cache (< 0: the current device): blocks of rows it used, and lanes its pass 2 cleared
     * from the rows' input masks because their record can never be taken.  Needs RRT_ENABLE_TEST_HOOKS=1 in the environment;
     * waits for the cache's launches. */
    int (*march_cache_fill)(int device, unsigned* blocks, unsigned long long* pruned_lanes);
    /* the grid (workgroups of 256) of the replays' pass 2 in `device`'s march cache (< 0: the current device), in place of the one
     * sized from the occupancy query: a replaying wave takes blocks of rows from a cursor, so any grid serves the same bytes.
     * 0 restores the sized grid.  Stays until changed, across keys and releases.  Needs RRT_ENABLE_TEST_HOOKS=1. */
    int (*replay_grid)(int device, unsigned blocks);
} rrt_test_records_table;

extern const rrt_test_records_table rrt_test_records;

#ifdef __cplusplus
}
#endif

#endif
