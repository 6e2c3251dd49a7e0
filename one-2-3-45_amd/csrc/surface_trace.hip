// Surface renderer: depth, hit point and kind per ray by an exhaustive fixed-stride march through the trilinear R^3 SDF lattice, with an exact
// empty-space skip; pinhole rays and the image packer.  Equal to the host twin (surface.py: trace_rays, brick_flags, camera_rays, pack_images) to the last
// bit: everything is fp64, one operation at a time, in a defined order (-ffp-contract=off); the trace has no square root.
//
// Definitions (R = grid_R, bmin / bmax the float32 bounds widened to fp64, ext = bmax - bmin, u float32 [R,R,R] x-major)
//   field      g(node) = double(u) - level, or level - double(u) with inside_positive; a value is OUTSIDE iff it is > 0.
//   ray        o, d float32 widened.  Per axis k: d_k == 0 constrains nothing when bmin_k <= o_k <= bmax_k, else the ray misses the box; d_k != 0:
//              a = (bmin_k - o_k) / d_k, b = (bmax_k - o_k) / d_k, low = min, high = max.  t0 = max(near, lows), t1 = min(far, highs); not t0 <= t1 is a
//              box miss.  A non-finite o or d is a BAD ray: counted, never dereferenced.
//   samples    h = stride * min_k(ext_k) / (R - 1) (computed on the host); n = floor((t1 - t0) / h), n > 2^20 is a bad ray; t_j = t0 + j h (a product,
//              not a running sum) for j = 0 .. n, and one more sample at t1 when t_n < t1.
//   value      p_k = o_k + t d_k; x_k = (p_k - bmin_k) / ext_k * (R - 1), clamped to [0, R - 1] (a NaN clamps to 0); i_k = min(floor(x_k), R - 2),
//              f_k = x_k - i_k; v = sum over the eight corners of ((wx wy) wz) g(corner), w = f or 1 - f, dx outer, dy, dz inner, from 0, left to right.
//   bricks     8 x 8 x 8 cells; flag[b] = 1 iff a node with index in [8 b_k, min(8 b_k + 8, R - 1)] on every axis fails g > 0 (NaN sets it).  A sample
//              whose cell lies in a brick with flag 0 is outside without a lookup: with all eight corners > 0 the sum above is a sum of non-negative
//              products of which one is >= g / 8 > 0, so the skip is exact in floating point; a skipped predecessor is evaluated when a bracket needs it.
//   march      j = the first sample that is not outside.  Its value NaN: STALLED.  j = 0: an entry hit at t0, kind 2.  Else lo = t_{j-1}, hi = t_j and
//              `refine` steps tm = lo + (hi - lo) * (s_lo / (s_lo - s_hi)) (even) or lo + (hi - lo) * 0.5 (odd); an outside value at tm replaces lo,
//              anything else hi; depth = lo + (hi - lo) * (s_lo / (s_lo - s_hi)), kind 1; a non-finite depth (infinite lattice values) is stalled too.
//              No such j: a miss.  depth = float32(t), point_k = float32(o_k + t d_k); both 0 for kind 0.
// Hit slots are appended to a list through a ballot and one integer atomicAdd per wave: its order changes between runs, its content does not, and nothing
// reads its order (the network kernels scatter through it).  Counters are integer atomics of wave sums.  No float atomics.
#include "mesh_math.h"
#include <float.h>

namespace o2345 {

constexpr int SURF_BRICK = 8;
constexpr int SURF_MAX_STEPS = 1 << 20;
constexpr int SURF_MAX_R = 2048;

struct SurfFrame {
    double bmin[3], bmax[3], ext[3];
    double rm1, h, t_near, t_far, level;
    int R, nb, refine, inside_positive;
};

__device__ __forceinline__ double surf_node(const float* __restrict__ u, long long i, const SurfFrame& f) {
    const double g = (double)u[i];
    return f.inside_positive ? f.level - g : g - f.level;
}

// the cell and the fractions of the sample at t; every index is in [0, R - 2] whatever t is
__device__ __forceinline__ void surf_cell(const SurfFrame& f, const double (&o)[3], const double (&d)[3], double t, int (&i)[3], double (&fr)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double p = o[k] + t * d[k];
        double x = (p - f.bmin[k]) / f.ext[k] * f.rm1;
        x = x > 0.0 ? x : 0.0;
        x = x < f.rm1 ? x : f.rm1;
        const int c = (int)x;                               // x >= 0: truncation is floor
        i[k] = c < f.R - 2 ? c : f.R - 2;
        fr[k] = x - (double)i[k];
    }
}

__device__ __forceinline__ double surf_value(const float* __restrict__ u, const SurfFrame& f, const int (&i)[3], const double (&fr)[3]) {
    double v = 0.0;
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
        const double wx = dx ? fr[0] : 1.0 - fr[0];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const double wy = dy ? fr[1] : 1.0 - fr[1];
            const long long row = ((long long)(i[0] + dx) * f.R + (i[1] + dy)) * f.R + i[2];
#pragma unroll
            for (int dz = 0; dz < 2; ++dz) {
                const double wz = dz ? fr[2] : 1.0 - fr[2];
                v = v + ((wx * wy) * wz) * surf_node(u, row + dz, f);
            }
        }
    }
    return v;
}

// one wave per brick: its (up to) 9^3 nodes in strides of 64, one ballot
__global__ __launch_bounds__(256) void k_surface_bricks(const float* __restrict__ u, SurfFrame f, uint8_t* __restrict__ flags) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nb = f.nb;
    if (b >= nb * nb * nb) return;                                   // the whole wave
    const int b0 = b / (nb * nb), b1 = b / nb % nb, b2 = b % nb;
    bool bad = false;
    for (int i = lane_id(); i < 729; i += 64) {
        const int x = SURF_BRICK * b0 + i / 81, y = SURF_BRICK * b1 + i / 9 % 9, z = SURF_BRICK * b2 + i % 9;
        if (x < f.R && y < f.R && z < f.R) bad |= !(surf_node(u, ((long long)x * f.R + y) * f.R + z, f) > 0.0);
    }
    const unsigned long long m = __ballot(bad);
    if (lane_id() == 0) flags[b] = m ? 1 : 0;
}

// One ray per lane, the whole march in registers.  img_w > 0: a wave takes an 8 x 8 pixel tile of the img_h x img_w image (lanes of similar march
// length together), else 64 consecutive rays.  flags null: no skip.
__global__ __launch_bounds__(256) void k_surface_trace(const float* __restrict__ u, const uint8_t* __restrict__ flags, const float* __restrict__ rays_o,
                                                       const float* __restrict__ rays_d, long long n, int img_h, int img_w, SurfFrame f,
                                                       float* __restrict__ depth, uint8_t* __restrict__ kind, float* __restrict__ point,
                                                       int* __restrict__ list, O2345SurfaceStats* __restrict__ st) {
    long long r;
    bool valid;
    if (img_w > 0) {
        const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
        const int tiles_x = (img_w + 7) >> 3;
        const long long px = wave % tiles_x * 8 + (lane_id() & 7), py = wave / tiles_x * 8 + (lane_id() >> 3);
        valid = px < img_w && py < img_h;
        r = py * img_w + px;
    } else {
        r = (long long)blockIdx.x * 256 + threadIdx.x;
        valid = r < n;
    }
    valid = valid && r < n;
    enum { NONE, HIT, ENTRY, BOX_MISS, MISS, STALLED, BAD };
    int what = NONE, samples = 0, lookups = 0;
    double t_hit = 0.0, o[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0};
    if (valid) {
        bool ray_finite = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = (double)rays_o[3 * r + k];
            d[k] = (double)rays_d[3 * r + k];
            ray_finite = ray_finite && finite(o[k]) && finite(d[k]);
        }
        double t0 = f.t_near, t1 = f.t_far;
        bool miss = false;
        if (ray_finite) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (d[k] == 0.0) {
                    miss = miss || !(f.bmin[k] <= o[k] && o[k] <= f.bmax[k]);
                } else {
                    const double a = (f.bmin[k] - o[k]) / d[k], b = (f.bmax[k] - o[k]) / d[k];
                    const double lo = a < b ? a : b, hi = a < b ? b : a;
                    t0 = lo > t0 ? lo : t0;
                    t1 = hi < t1 ? hi : t1;
                }
            }
            miss = miss || !(t0 <= t1);
        }
        const double q = floor((t1 - t0) / f.h);
        if (!ray_finite) what = BAD;
        else if (miss) what = BOX_MISS;
        else if (!(q <= (double)SURF_MAX_STEPS)) what = BAD;
        else {
            const int ns = (int)q;
            const int m = ns + 1 + ((t0 + (double)ns * f.h) < t1 ? 1 : 0);
            int i[3];
            double fr[3];
            double pt = 0.0, ps = 0.0, v = 0.0, t = t0;
            bool pskip = false, found = false;
            int j = 0;
            for (; j < m; ++j) {
                t = j <= ns ? t0 + (double)j * f.h : t1;
                surf_cell(f, o, d, t, i, fr);
                ++samples;
                const bool ev = !flags || flags[((i[0] >> 3) * f.nb + (i[1] >> 3)) * f.nb + (i[2] >> 3)] != 0;
                if (ev) {
                    v = surf_value(u, f, i, fr);
                    ++lookups;
                    if (!(v > 0.0)) { found = true; break; }
                }
                pt = t; ps = v; pskip = !ev;
            }
            if (!found) what = MISS;
            else if (v != v) what = STALLED;
            else if (j == 0) { what = ENTRY; t_hit = t0; }
            else {
                if (pskip) {
                    surf_cell(f, o, d, pt, i, fr);
                    ps = surf_value(u, f, i, fr);
                    ++lookups;
                }
                double lo = pt, hi = t, s_lo = ps, s_hi = v;
                for (int step = 0; step < f.refine; ++step) {
                    const double tm = (step & 1) ? lo + (hi - lo) * 0.5 : lo + (hi - lo) * (s_lo / (s_lo - s_hi));
                    surf_cell(f, o, d, tm, i, fr);
                    const double vm = surf_value(u, f, i, fr);
                    ++samples; ++lookups;
                    if (vm > 0.0) { lo = tm; s_lo = vm; } else { hi = tm; s_hi = vm; }
                }
                t_hit = lo + (hi - lo) * (s_lo / (s_lo - s_hi));
                what = finite(t_hit) ? HIT : STALLED;
            }
        }
        const bool hit = what == HIT || what == ENTRY;
        depth[r] = hit ? (float)t_hit : 0.f;
        kind[r] = what == HIT ? 1 : what == ENTRY ? 2 : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) point[3 * r + k] = hit ? (float)(o[k] + t_hit * d[k]) : 0.f;
    }
    // every lane of the wave from here on
    const bool hit = what == HIT || what == ENTRY;
    int total;
    const int pos = wave_prefix(hit, total);
    int base = 0;
    if (lane_id() == 0 && total) base = atomicAdd(&st->n_list, total);
    base = __shfl(base, 0);
    if (hit && (long long)base + pos < n) list[base + pos] = (int)r;      // always in range: every ray is listed at most once
    wave_count(what == HIT, &st->hits);
    wave_count(what == ENTRY, &st->entry_hits);
    wave_count(what == BOX_MISS, &st->box_misses);
    wave_count(what == MISS, &st->misses);
    wave_count(what == STALLED, &st->stalled);
    wave_count(what == BAD, &st->bad_rays);
    samples = wave_sum(samples);                                      // <= 64 x (2^20 + 34)
    lookups = wave_sum(lookups);
    if (lane_id() == 0) {
        if (samples) atomicAdd(&st->samples, (unsigned long long)samples);
        if (lookups) atomicAdd(&st->lookups, (unsigned long long)lookups);
    }
}

struct CamFrame {
    double fx, fy, cx, cy;
    double M[12];                                          // rows 0 .. 2 of c2w
};

// thread per pixel, raster order
__global__ __launch_bounds__(256) void k_camera_rays(CamFrame c, int H, int W, float* __restrict__ rays_o, float* __restrict__ rays_d) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long)H * W) return;
    const int py = (int)(p / W), px = (int)(p % W);
    const double v[3] = {((double)px - c.cx) / c.fx, ((double)py - c.cy) / c.fy, 1.0};
    double n[3];
    (void)unit_normal(v, n);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        rays_d[3 * p + r] = (float)((c.M[4 * r] * n[0] + c.M[4 * r + 1] * n[1]) + c.M[4 * r + 2] * n[2]);
        rays_o[3 * p + r] = (float)c.M[4 * r + 3];
    }
}

// thread per pixel, raster order; rgb and grad are read at hits only
__global__ __launch_bounds__(256) void k_surface_pack(const uint8_t* __restrict__ kind, const float* __restrict__ depth, const float* __restrict__ rgb,
                                                      const float* __restrict__ grad, long long n, uchar4 background, uchar4* __restrict__ color,
                                                      uchar4* __restrict__ normal, float* __restrict__ depth_out) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    uchar4 c = background, q = make_uchar4(0, 0, 0, 0);
    float z = 0.f;
    if (kind[p] != 0) {
        c = make_uchar4(mesh_colour_u8(rgb[3 * p]), mesh_colour_u8(rgb[3 * p + 1]), mesh_colour_u8(rgb[3 * p + 2]), 255);
        const double g[3] = {(double)grad[3 * p], (double)grad[3 * p + 1], (double)grad[3 * p + 2]};
        double m[3];
        (void)unit_normal(g, m);
        q = make_uchar4(mesh_colour_u8((float)(m[0] * 0.5 + 0.5)), mesh_colour_u8((float)(m[1] * 0.5 + 0.5)), mesh_colour_u8((float)(m[2] * 0.5 + 0.5)), 255);
        z = depth[p];
    }
    color[p] = c;
    normal[p] = q;
    depth_out[p] = z;
}

static bool surf_rays_ok(long long n) { return n >= 0 && n < (1ll << 31); }

// the one walk through the workspace: carves it, or sizes it when ws is null; returns its size
static size_t surf_carve(void* ws, long long n, int*& list) {
    Carver w(ws);
    list = w.take<int>(n);
    return w.bytes();
}

// the frame of a call from the C ABI's host arrays; false with the error set
static bool surf_frame(const char* unit, int grid_R, double level, int inside_positive, const float* bound_min, const float* bound_max, SurfFrame& f) {
    if (!(grid_R >= 2 && grid_R <= SURF_MAX_R)) { set_error("%s: resolution must be in [2, %d], got %d", unit, SURF_MAX_R, grid_R); return false; }
    if (!finite(level)) { set_error("%s: level must be finite, got %g", unit, level); return false; }
    f = SurfFrame{};
    f.R = grid_R;
    f.nb = (grid_R - 1 + SURF_BRICK - 1) / SURF_BRICK;
    f.rm1 = (double)grid_R - 1.0;
    f.level = level;
    f.inside_positive = inside_positive ? 1 : 0;
    for (int k = 0; k < 3; ++k) {
        f.bmin[k] = bound_min ? (double)bound_min[k] : -1.0;
        f.bmax[k] = bound_max ? (double)bound_max[k] : 1.0;
        f.ext[k] = f.bmax[k] - f.bmin[k];
        if (!(f.ext[k] > 0.0 && finite(f.ext[k]) && finite(f.bmin[k]))) {
            set_error("%s: bound_max must be above bound_min on every axis, both finite", unit);
            return false;
        }
    }
    return true;
}

}  // namespace o2345

using namespace o2345;

extern "C" {

int o2345_surface_bricks(const float* u, int grid_R, double level, int inside_positive, uint8_t* flags, void* stream) {
    SurfFrame f;
    if (!surf_frame("surface_bricks", grid_R, level, inside_positive, nullptr, nullptr, f)) return -1;
    O2345_REQUIRE(u && flags, "surface_bricks: null pointer");
    hipLaunchKernelGGL(k_surface_bricks, dim3(cdiv((long long)f.nb * f.nb * f.nb, 4)), dim3(256), 0, (hipStream_t)stream, u, f, flags);
    return check_launch("surface_bricks");
}

size_t o2345_surface_trace_workspace_bytes(long long n) {
    if (!surf_rays_ok(n)) return 0;
    int* list;
    const size_t b = surf_carve(nullptr, n, list);
    return b ? b : 16;
}

int o2345_surface_trace(const float* u, int grid_R, const uint8_t* flags, const float* rays_o, const float* rays_d, long long n, int img_h, int img_w,
                        double t_near, double t_far, double stride, int refine, double level, int inside_positive, const float* bound_min,
                        const float* bound_max, void* workspace, size_t workspace_bytes, float* depth, uint8_t* kind, float* point,
                        O2345SurfaceStats* stats, void* stream) {
    SurfFrame f;
    O2345_REQUIRE(bound_min && bound_max && stats && workspace && u, "surface_trace: null pointer");
    if (!surf_frame("surface_trace", grid_R, level, inside_positive, bound_min, bound_max, f)) return -1;
    O2345_REQUIRE(surf_rays_ok(n), "surface_trace: bad size (n must be in [0, 2^31))");
    O2345_REQUIRE(n == 0 || (rays_o && rays_d && depth && kind && point), "surface_trace: null pointer");
    O2345_REQUIRE(stride > 0.0 && stride <= 8.0, "surface_trace: stride must be in (0, 8], got %g", stride);
    O2345_REQUIRE(refine >= 0 && refine <= 32, "surface_trace: refine must be in [0, 32], got %d", refine);
    O2345_REQUIRE(o2345::finite(t_near) && o2345::finite(t_far), "surface_trace: near and far must be finite");
    O2345_REQUIRE((img_h == 0 && img_w == 0) || (img_h > 0 && img_w > 0 && (long long)img_h * img_w == n),
                  "surface_trace: img_h x img_w must be 0 x 0 or the ray count, got %d x %d for %lld rays", img_h, img_w, n);
    O2345_REQUIRE(workspace_bytes >= o2345_surface_trace_workspace_bytes(n), "surface_trace: workspace too small");
    O2345_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)stats & 7) == 0, "surface_trace: workspace must be 16-byte and stats 8-byte aligned");
    f.refine = refine;
    f.t_near = t_near;
    f.t_far = t_far;
    double mn = f.ext[0];
    for (int k = 1; k < 3; ++k) mn = f.ext[k] < mn ? f.ext[k] : mn;
    f.h = stride * mn / f.rm1;
    O2345_REQUIRE(f.h > 0.0 && f.h <= DBL_MAX, "surface_trace: the step %g is not a positive finite number", f.h);
    int* list;
    (void)surf_carve(workspace, n, list);
    hipStream_t s = (hipStream_t)stream;
    O2345_HIP(hipMemsetAsync(stats, 0, sizeof *stats, s));
    if (n == 0) return 0;
    const long long blocks = img_w > 0 ? cdiv((long long)((img_w + 7) / 8) * ((img_h + 7) / 8), 4) : cdiv(n, 256);
    hipLaunchKernelGGL(k_surface_trace, dim3((unsigned)blocks), dim3(256), 0, s, u, flags, rays_o, rays_d, n, img_h, img_w, f, depth, kind, point, list,
                       stats);
    return check_launch("surface_trace");
}

int o2345_camera_rays(const float* K_host, const float* c2w_host, int H, int W, float* rays_o, float* rays_d, void* stream) {
    O2345_REQUIRE(K_host && c2w_host && rays_o && rays_d, "camera_rays: null pointer");
    O2345_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), "camera_rays: bad image size %d x %d", H, W);
    bool finite = true;
    for (int k = 0; k < 9; ++k) finite = finite && fabsf(K_host[k]) <= FLT_MAX;
    for (int k = 0; k < 12; ++k) finite = finite && fabsf(c2w_host[k]) <= FLT_MAX;
    O2345_REQUIRE(finite, "camera_rays: K and c2w must be finite");
    O2345_REQUIRE(K_host[1] == 0.f && K_host[3] == 0.f && K_host[6] == 0.f && K_host[7] == 0.f && K_host[8] == 1.f && K_host[0] != 0.f && K_host[4] != 0.f,
                  "camera_rays: a pinhole camera without skew is [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] with fx, fy != 0");
    CamFrame c;
    c.fx = (double)K_host[0]; c.fy = (double)K_host[4]; c.cx = (double)K_host[2]; c.cy = (double)K_host[5];
    for (int k = 0; k < 12; ++k) c.M[k] = (double)c2w_host[k];
    hipLaunchKernelGGL(k_camera_rays, dim3(cdiv((long long)H * W, 256)), dim3(256), 0, (hipStream_t)stream, c, H, W, rays_o, rays_d);
    return check_launch("camera_rays");
}

int o2345_surface_pack(const uint8_t* kind, const float* depth, const float* rgb, const float* grad, int H, int W, const uint8_t* background_host,
                       uint8_t* color, uint8_t* normal, float* depth_out, void* stream) {
    O2345_REQUIRE(kind && depth && rgb && grad && background_host && color && normal && depth_out, "surface_pack: null pointer");
    O2345_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), "surface_pack: bad image size %d x %d", H, W);
    O2345_REQUIRE(((uintptr_t)color & 3) == 0 && ((uintptr_t)normal & 3) == 0, "surface_pack: the images must be 4-byte aligned");
    const uchar4 bg = make_uchar4(background_host[0], background_host[1], background_host[2], background_host[3]);
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(k_surface_pack, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, kind, depth, rgb, grad, n, bg, (uchar4*)color, (uchar4*)normal,
                       depth_out);
    return check_launch("surface_pack");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_surface_trace() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)k_surface_trace);
}
}  // namespace o2345
