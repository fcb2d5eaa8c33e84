/*
 * rrt_projection.h -- the primary ray of a panorama's virtual pixel (include/rrt.h: rrt_projection has the contract), as ONE
 * __host__ __device__ function: panorama_pixels and projection_map (rrt_kernels.h) run it on the device, rrt_projection_ray
 * (rrt_hip.hip's C ABI) on the host, so the tests can demand that the host query and the device agree bit for bit.  Both passes
 * of rrt_hip.hip are built with -ffp-contract=off, and `/` and sqrtf are correctly rounded in both (hipcc's default for device
 * code): the same source gives the same bits.
 *
 * A SECTION of rrt_hip.hip, included by rrt_kernels.h inside its anonymous namespace.
 */
#ifndef RRT_PROJECTION_H
#define RRT_PROJECTION_H

/* what the kernel needs of an rrt_projection, by value beside FrameArgs: the kind and the half-spans in radians (fisheye: a_h = a) */
struct ProjArgs { int kind; float a_h, a_v; };

/* The unit direction of virtual pixel (x, y) of the W x H frame, before any nudge (dir = 0 and false: a fisheye sub-sample outside
 * the disc).  D = fw*A + (rt*B + up*C) per component, as primary_ray forms the pinhole's fw + (rt*u + up*v) -- RRT_PROJ_PINHOLE is
 * that ray without the lens (A = 1 is exact) -- then raymarcher.cu's normalize (rrt_device.h: normalize). */
__host__ __device__ __forceinline__ bool projection_dir(const ProjArgs& pj, int W, int H, int x, int y, const rrt_camera& c,
                                                        float dir[3]) {
    float A, B, C;
    if (pj.kind == RRT_PROJ_EQUIRECT) {
        const float lon = (((float)x + 0.5f) / (float)W * 2.0f - 1.0f) * pj.a_h;
        const float lat = (((float)y + 0.5f) / (float)H * 2.0f - 1.0f) * pj.a_v;
        float s_lat, c_lat, s_lon, c_lon;
        rrt_sincosf(lat, &s_lat, &c_lat);
        rrt_sincosf(lon, &s_lon, &c_lon);
        A = c_lat * c_lon; B = c_lat * s_lon; C = s_lat;
    } else if (pj.kind == RRT_PROJ_FISHEYE) {
        const float u = (2.0f * ((float)x + 0.5f) - (float)W) / (float)H;
        const float v = (2.0f * ((float)y + 0.5f) - (float)H) / (float)H;
        const float r2 = u * u + v * v;
        if (r2 > 1.0f) { dir[0] = 0.0f; dir[1] = 0.0f; dir[2] = 0.0f; return false; }
        const float r = sqrtf(r2);
        float s_t, c_t;
        rrt_sincosf(r * pj.a_h, &s_t, &c_t);
        const float k = r > 0.0f ? s_t / r : 0.0f;
        A = c_t; B = u * k; C = v * k;
    } else {                                    /* raymarcher.cu:20-34 without the lens */
        const float uvx = (float)x / (float)W, uvy = (float)y / (float)H;
        float u = uvx * 2.0f - 1.0f;
        const float v = uvy * 2.0f - 1.0f;
        u *= (float)W / (float)H;
        A = 1.0f; B = u; C = v;
    }
    float d[3];
    for (int i = 0; i < 3; ++i) d[i] = c.forward[i] * A + (c.right[i] * B + c.up[i] * C);
    const float mag = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (mag < 1e-6f) { dir[0] = 0.0f; dir[1] = 0.0f; dir[2] = 0.0f; return true; }
    for (int i = 0; i < 3; ++i) dir[i] = d[i] / mag;
    return true;
}

#endif /* RRT_PROJECTION_H */
