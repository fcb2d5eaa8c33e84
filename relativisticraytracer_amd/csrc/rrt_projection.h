/*
 * rrt_projection.h -- the primary ray of a panorama's virtual pixel (include/rrt.h: rrt_projection has the contract), as ONE
 * __host__ __device__ function: panorama_pixels and projection_map (rrt_kernels.h) run it on the device, rrt_projection_ray
 * (rrt_hip.hip's C ABI) on the host, so the tests can demand that the host query and the device agree bit for bit.  Both passes
 * of rrt_hip.hip are built with -ffp-contract=off, and `/` and sqrtf are correctly rounded in both (hipcc's default for device
 * code): the same source gives the same bits.
 *
 * stereo_ray, the primary ray of a stereo frame's eye (rrt_stereo), is built on the same pieces: stereo_pixels and rrt_stereo_ray.
 * lens_ray, the primary ray through a point of a thin lens (rrt_launch_raymarch_dof), likewise: lens_pixels and rrt_lens_ray.
 *
 * A SECTION of rrt_hip.hip, included by rrt_kernels.h inside its anonymous namespace.
 */
#ifndef RRT_PROJECTION_H
#define RRT_PROJECTION_H

/* what the kernel needs of an rrt_projection, by value beside FrameArgs: the kind and the half-spans in radians (fisheye: a_h = a) */
struct ProjArgs { int kind; float a_h, a_v; };

/* an equirect pixel's latitude and the sines and cosines of its latitude and longitude */
struct EquirectAngles { float lat, s_lat, c_lat, s_lon, c_lon; };
__host__ __device__ __forceinline__ EquirectAngles equirect_angles(const ProjArgs& pj, int W, int H, int x, int y) {
    EquirectAngles e;
    const float lon = (((float)x + 0.5f) / (float)W * 2.0f - 1.0f) * pj.a_h;
    e.lat = (((float)y + 0.5f) / (float)H * 2.0f - 1.0f) * pj.a_v;
    rrt_sincosf(e.lat, &e.s_lat, &e.c_lat);
    rrt_sincosf(lon, &e.s_lon, &e.c_lon);
    return e;
}

/* dir = normalize(D), D = fw*A + (rt*B + up*C) per component (raymarcher.cu's normalize: rrt_device.h, 1e-6f guard) -- the tail of
 * projection_dir, which spells it out itself: calling this from there gives the existing kernels another register allocation */
__host__ __device__ __forceinline__ void basis_dir(const rrt_camera& c, float A, float B, float C, float dir[3]) {
    float d[3];
    for (int i = 0; i < 3; ++i) d[i] = c.forward[i] * A + (c.right[i] * B + c.up[i] * C);
    const float mag = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (mag < 1e-6f) { dir[0] = 0.0f; dir[1] = 0.0f; dir[2] = 0.0f; return; }
    for (int i = 0; i < 3; ++i) dir[i] = d[i] / mag;
}

/* The unit direction of virtual pixel (x, y) of the W x H frame, before any nudge (dir = 0 and false: a fisheye sub-sample outside
 * the disc).  D = fw*A + (rt*B + up*C) per component, as primary_ray forms the pinhole's fw + (rt*u + up*v) -- RRT_PROJ_PINHOLE is
 * that ray without the lens (A = 1 is exact) -- then raymarcher.cu's normalize (rrt_device.h: normalize). */
__host__ __device__ __forceinline__ bool projection_dir(const ProjArgs& pj, int W, int H, int x, int y, const rrt_camera& c,
                                                        float dir[3]) {
    float A, B, C;
    if (pj.kind == RRT_PROJ_EQUIRECT) {
        const EquirectAngles e = equirect_angles(pj, W, H, x, y);
        A = e.c_lat * e.c_lon; B = e.c_lat * e.s_lon; C = e.s_lat;
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

/* what the kernel needs of an rrt_stereo, by value beside ProjArgs (include/rrt.h has the contract): the eye's virtual frame, which
 * composite half is the right eye, hb and the merge latitudes in radians (equirect), and per eye the pinhole's k = e*hb and
 * c = k / convergence -- all rounded on the host */
struct StereoArgs {
    int W, H;                   /* one eye's virtual frame: s*width x s*height */
    int right_x, right_y;       /* the right eye's half: virtual x >= right_x and y >= right_y (the other one 0) */
    float hb, from, to;
    float k_left, k_right, c_left, c_right;
};

/* The primary ray of eye `eye`'s virtual pixel (x, y): origin org, unit direction dir (before any nudge) and -- pinhole -- the uv
 * the vignette reads (after the lens, as primary_ray returns it; equirect: 0).  use_lens / lens_k: rrt_effects' lens, pinhole only
 * (the host query passes 0).  k == 0 and c == 0 add nothing (the zero rule): base 0 is the mono frame's ray bit for bit. */
__host__ __device__ __forceinline__ void stereo_ray(const ProjArgs& pj, const StereoArgs& sa, int eye, int x, int y,
                                                    const rrt_camera& c, int use_lens, float lens_k, float org[3], float dir[3],
                                                    float& uvx, float& uvy) {
    float k, R[3];
    if (pj.kind == RRT_PROJ_EQUIRECT) {         /* ODS: projection_dir's ray from a point on the circle of radius hb */
        const EquirectAngles e = equirect_angles(pj, sa.W, sa.H, x, y);
        basis_dir(c, e.c_lat * e.c_lon, e.c_lat * e.s_lon, e.s_lat, dir);
        const float a = fabsf(e.lat);
        const float f = a <= sa.from ? 1.0f : (a >= sa.to ? 0.0f : (sa.to - a) / (sa.to - sa.from));
        k = f * sa.hb;
        if (eye == RRT_EYE_LEFT) k = -k;
        for (int i = 0; i < 3; ++i) R[i] = c.right[i] * e.c_lon - c.forward[i] * e.s_lon;
        uvx = 0.0f; uvy = 0.0f;
    } else {                                    /* off-axis pinhole: primary_ray (raymarcher.cu:20-34, lens included) with u - c */
        uvx = (float)x / (float)sa.W;
        uvy = (float)y / (float)sa.H;
        if (use_lens) {                         /* rrt_device.h: lens_distort */
            const float tx = uvx - 0.5f, ty = uvy - 0.5f;
            const float r2 = tx * tx + ty * ty;
            const float f = 1.0f + r2 * lens_k;
            uvx = tx * f + 0.5f;
            uvy = ty * f + 0.5f;
        }
        float u = uvx * 2.0f - 1.0f;
        const float v = uvy * 2.0f - 1.0f;
        const float aspect = (float)sa.W / (float)sa.H;
        u *= aspect;
        const float cc = eye == RRT_EYE_LEFT ? sa.c_left : sa.c_right;
        if (cc != 0.0f) u = u - cc;
        basis_dir(c, 1.0f, u, v, dir);          /* fw*1 == fw: primary_ray's fw + (rt*u + up*v) */
        k = eye == RRT_EYE_LEFT ? sa.k_left : sa.k_right;
        for (int i = 0; i < 3; ++i) R[i] = c.right[i];
    }
    if (k != 0.0f) for (int i = 0; i < 3; ++i) org[i] = c.pos[i] + R[i] * k;
    else for (int i = 0; i < 3; ++i) org[i] = c.pos[i];
}

/* The primary ray of virtual pixel (x, y) of the W x H frame seen through the lens point (lx, ly) of a thin lens focused at `focus`
 * (rrt_launch_raymarch_dof, include/rrt.h has the contract; cx = lx / focus and cy = ly / focus are rounded on the host): stereo_ray's
 * off-axis pinhole on two axes -- primary_ray (raymarcher.cu:20-34, lens distortion included) with u - cx and v - cy, from
 * pos + rt*lx + up*ly.  org, the unit direction dir (before any nudge) and the uv the vignette reads.  Zero rule: a zero cx or cy
 * leaves its coordinate untouched and a zero lx or ly adds nothing, so the lens point (0, 0) is primary_ray bit for bit and
 * (k, 0) is stereo_ray's eye.  lens_pixels and rrt_lens_ray (which passes use_lens = 0). */
__host__ __device__ __forceinline__ void lens_ray(int W, int H, int x, int y, const rrt_camera& c, int use_lens, float lens_k,
                                                  float lx, float ly, float cx, float cy, float org[3], float dir[3], float& uvx,
                                                  float& uvy) {
    uvx = (float)x / (float)W;
    uvy = (float)y / (float)H;
    if (use_lens) {                             /* rrt_device.h: lens_distort */
        const float tx = uvx - 0.5f, ty = uvy - 0.5f;
        const float r2 = tx * tx + ty * ty;
        const float f = 1.0f + r2 * lens_k;
        uvx = tx * f + 0.5f;
        uvy = ty * f + 0.5f;
    }
    float u = uvx * 2.0f - 1.0f;
    float v = uvy * 2.0f - 1.0f;
    const float aspect = (float)W / (float)H;
    u *= aspect;
    if (cx != 0.0f) u = u - cx;
    if (cy != 0.0f) v = v - cy;
    basis_dir(c, 1.0f, u, v, dir);              /* fw*1 == fw: primary_ray's fw + (rt*u + up*v) */
    for (int i = 0; i < 3; ++i) org[i] = c.pos[i];
    if (lx != 0.0f) for (int i = 0; i < 3; ++i) org[i] = org[i] + c.right[i] * lx;
    if (ly != 0.0f) for (int i = 0; i < 3; ++i) org[i] = org[i] + c.up[i] * ly;
}

/* rrt_lens_points (host only; include/rrt.h): n lens points on a disc of radius `aperture` into xy[2 n] -- (0, 0) for n = 1, else
 * Vogel's spiral in double (equal-area rings, the golden angle between neighbours), rounded to float.  false: refused. */
inline bool lens_points(float aperture, int n, float rotation, float* xy) {
    if (!xy || !(n == 1 || n == 2 || n == 4 || n == 8 || n == 16)) return false;
    if (!std::isfinite(aperture) || aperture < 0.0f || !std::isfinite(rotation)) return false;
    if (n == 1) { xy[0] = 0.0f; xy[1] = 0.0f; return true; }
    const double golden = 3.14159265358979323846 * (3.0 - std::sqrt(5.0));
    for (int k = 0; k < n; ++k) {
        const double r = (double)aperture * std::sqrt(((double)k + 0.5) / (double)n);
        const double th = (double)rotation + (double)k * golden;
        xy[2 * k] = (float)(r * std::cos(th));
        xy[2 * k + 1] = (float)(r * std::sin(th));
    }
    return true;
}

#endif /* RRT_PROJECTION_H */
