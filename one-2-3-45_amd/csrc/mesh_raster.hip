// A triangle rasterizer on the device: depth, barycentrics and face id per pixel of a mesh seen from a pinhole camera, and the per-pixel colour and normal
// that o2345_surface_pack turns into images.  Every output equals the host twin (one-2-3-45_amd/raster.py) to the last bit: coverage is decided in 64-bit
// integers on corners snapped to 1/256 pixel, depth is fp64 computed one operation at a time (mesh_raster_math.h), visibility is an fp64 comparison with
// ties to the smaller face index -- nothing depends on face order, binning, tile size or run.  include/o2345.h has the definition.
//
// Organisation (nothing about its speed has been measured)
//   k_rs_setup   one thread per face: corners to the screen, the class, the pixel box (RsFace, 80 bytes, in the workspace); a face that takes part adds 1
//                to the count of every 8 x 8-pixel tile its box touches (integer atomics).  The box is conservative: a thin diagonal face is listed in
//                tiles it does not cover, and a face that fills the screen is listed in every tile -- the lists are sized by the counted total.
//   scan         the tile counts -> the start of every tile's list (mesh_common.h's three-launch scan).
//   k_rs_setup   (emit, FILL) the same walk again, writing the face at tile_start + cursor++.  The order inside a list is arbitrary and does not matter.
//   k_rs_tiles   one wave per tile, one lane per pixel (the arrangement of surface_trace.hip).  The list is staged through LDS 64 faces at a time, one
//                face per lane; then every lane walks the batch and keeps its own (z, face) minimum in registers.  No atomics on pixels.
//   k_rs_shade   one thread per pixel: colour and normal from face + bary.
//   k_rs_shade_tex  one thread per pixel: the textured asset's shading from face + bary (mesh_raster_tex_math.h): albedo from the atlas, the normal from
//                the normal map through the file's tangent frame, a headlight-lit colour.  Four (with the map eight) 4-byte texel loads per pixel straight
//                from memory, nothing staged in LDS; one ballot per counter and wave.
// No kernel waits for another workgroup.  Bad input never faults: an index outside [0, nv) is counted and never dereferenced; list entries, list bounds and
// face ids are clamped to the sizes the caller states.
#include "mesh_common.h"
#include "mesh_raster_math.h"
#include "mesh_raster_tex_math.h"

namespace o2345 {

constexpr int RS_BATCH = 64;                          // faces staged per round: one per lane, 64 * 84 bytes of LDS
constexpr long long RS_MAX_PAIRS = 1ll << 31;

// device scalars of a call (workspace head)
struct RsTotals {
    unsigned long long skipped[RS_CLASSES];           // by class; [0] counts the faces that take part
    unsigned long long pairs, pixels;
    long long scan_total;
};
static_assert(sizeof(RsTotals) <= 128, "the head is 128 bytes");

__device__ __forceinline__ int rs_tiles_x(int W) { return (W + RS_TILE - 1) / RS_TILE; }

// FILL false: RsFace of every face, the class counts, the tile counts; true: the tile lists
template <typename IDX, bool FILL>
__global__ __launch_bounds__(256) void k_rs_setup(const double* __restrict__ verts, int nv, const IDX* __restrict__ tris, long long nt, RsCamera cam,
                                                  RsFace* __restrict__ faces, int* __restrict__ tile_count, const int* __restrict__ tile_start,
                                                  int* __restrict__ cursor, int* __restrict__ lists, long long n_pairs, RsTotals* __restrict__ tot) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    int cls = -1;
    unsigned long long pairs = 0;
    if (t < nt) {
        RsFace f;
        if (FILL) f = faces[t];
        else {
            int idx[3];
            const bool in_range = mesh_triangle(tris, t, nv, idx[0], idx[1], idx[2]);
            (void)rs_setup(cam, verts, in_range, idx, f);
            faces[t] = f;
        }
        cls = f.cls;
        if (cls == RS_OK) {
            // the box lies inside the image; the clamps hold for a workspace that pass 1 did not write, too
            const int tiles_x = rs_tiles_x(cam.W), tiles_y = rs_tiles_x(cam.H);
            const int tx0 = max(f.px0 / RS_TILE, 0), tx1 = min(f.px1 / RS_TILE, tiles_x - 1), ty0 = max(f.py0 / RS_TILE, 0), ty1 = min(f.py1 / RS_TILE, tiles_y - 1);
            pairs = tx1 >= tx0 && ty1 >= ty0 ? (unsigned long long)(tx1 - tx0 + 1) * (unsigned long long)(ty1 - ty0 + 1) : 0;
            for (int ty = ty0; ty <= ty1; ++ty)
                for (int tx = tx0; tx <= tx1; ++tx) {
                    const long long tile = (long long)ty * tiles_x + tx;
                    if (FILL) {
                        const long long at = (long long)tile_start[tile] + atomicAdd(cursor + tile, 1);
                        if (at >= 0 && at < n_pairs) lists[at] = (int)t;              // at < n_pairs unless the caller passed another count
                    } else atomicAdd(tile_count + tile, 1);
                }
        }
    }
    if (!FILL) {
#pragma unroll
        for (int k = 0; k < RS_CLASSES; ++k) wave_count(cls == k, &tot->skipped[k]);
        pairs = wave_sum(pairs);
        if (lane_id() == 0 && pairs) atomicAdd(&tot->pairs, pairs);
    }
}

// the counts, in the order of O2345_RASTER_*
__global__ __launch_bounds__(64) void k_rs_counts(const RsTotals* __restrict__ tot, long long* __restrict__ counts, int pixels_only) {
    if (blockIdx.x || threadIdx.x) return;
    counts[O2345_RASTER_PIXELS] = pixels_only ? (long long)tot->pixels : 0;
    if (pixels_only) return;
    for (int k = 1; k < RS_CLASSES; ++k) counts[k - 1] = (long long)tot->skipped[k];
    counts[O2345_RASTER_BINNED] = (long long)tot->skipped[RS_OK];
    counts[O2345_RASTER_PAIRS] = (long long)tot->pairs;
}

// one wave per tile, one lane per pixel
__global__ __launch_bounds__(64) void k_rs_tiles(const RsFace* __restrict__ faces, long long nt, const int* __restrict__ tile_start,
                                                 const int* __restrict__ tile_count, const int* __restrict__ lists, long long n_pairs, RsCamera cam,
                                                 int* __restrict__ face_out, float* __restrict__ depth, float* __restrict__ bary, RsTotals* __restrict__ tot) {
    __shared__ RsFace sh_face[RS_BATCH];
    __shared__ int sh_id[RS_BATCH];
    const int tiles_x = rs_tiles_x(cam.W);
    const int lane = threadIdx.x;
    const int px = (int)(blockIdx.x % tiles_x) * RS_TILE + (lane & 7), py = (int)(blockIdx.x / tiles_x) * RS_TILE + (lane >> 3);
    const bool in_image = px < cam.W && py < cam.H;
    long long begin = tile_start[blockIdx.x], end = begin + tile_count[blockIdx.x];
    begin = begin < 0 ? 0 : begin;
    end = end > n_pairs ? n_pairs : end;
    double best_z = (double)INFINITY, best_b[3] = {0.0, 0.0, 0.0};
    int best_f = -1, best_corner[3] = {0, 1, 2};
    for (long long base = begin; base < end; base += RS_BATCH) {
        const int n = (int)(end - base < RS_BATCH ? end - base : RS_BATCH);
        if (lane < n) {
            const int id = lists[base + lane];
            const bool ok = id >= 0 && id < nt;
            sh_id[lane] = ok ? id : -1;
            if (ok) sh_face[lane] = faces[id];
        }
        __syncthreads();
        if (in_image)
            for (int j = 0; j < n; ++j) {
                const int id = sh_id[j];
                if (id < 0) continue;
                const RsFace& f = sh_face[j];
                if (f.cls != RS_OK || px < f.px0 || px > f.px1 || py < f.py0 || py > f.py1) continue;
                long long w[3];
                if (!rs_edges(f, px, py, w)) continue;
                double z, b[3];
                if (!rs_depth(f, w, z, b)) continue;
                if (z < best_z || (z == best_z && id < best_f)) {
                    best_z = z; best_f = id;
#pragma unroll
                    for (int k = 0; k < 3; ++k) { best_b[k] = b[k]; best_corner[k] = f.corner[k]; }
                }
            }
        __syncthreads();
    }
    const bool hit = in_image && best_f >= 0;
    if (in_image) {
        const long long p = (long long)py * cam.W + px;
        float out[3] = {0.f, 0.f, 0.f};
        if (hit) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float v = (float)best_b[k];
                if (best_corner[k] == 0) out[0] = v; else if (best_corner[k] == 1) out[1] = v; else out[2] = v;
            }
        }
        face_out[p] = best_f;
        depth[p] = hit ? (float)rs_ray_depth(cam, px, py, best_z) : 0.f;
        bary[3 * p] = out[0]; bary[3 * p + 1] = out[1]; bary[3 * p + 2] = out[2];
    }
    wave_count(hit, &tot->pixels);
}

// What both shade kernels share.  The hit test: face t is a triangle of the mesh with its three indices in [0, nv) -> idx
template <typename IDX>
__device__ __forceinline__ bool rs_hit(const IDX* tris, long long nt, int nv, int t, int (&idx)[3]) { return t >= 0 && t < nt && mesh_triangle(tris, (long long)t, nv, idx[0], idx[1], idx[2]); }
// pixel p's float32 barycentrics, widened
__device__ __forceinline__ void rs_bary(const float* bary, long long p, double (&b)[3]) { b[0] = (double)bary[3 * p]; b[1] = (double)bary[3 * p + 1]; b[2] = (double)bary[3 * p + 2]; }
// the flat (P1 - P0) x (P2 - P0) of the fp64 vertices, rounded to float32 once
__device__ __forceinline__ void rs_flat_normal_f32(const double* verts, const int (&idx)[3], float (&m)[3]) {
    double P[3][3], g[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) P[k / 3][k % 3] = verts[3 * (long long)idx[k / 3] + k % 3];
    rs_flat_normal(P, g);
    m[0] = (float)g[0]; m[1] = (float)g[1]; m[2] = (float)g[2];
}
// pixel p's outputs; l, lit: the textured stage's fourth image, or null
__device__ __forceinline__ void rs_store(long long p, bool hit, const float (&c)[3], const float (&m)[3], const float* l, unsigned char* kind, float* rgb, float* nrm, float* lit) {
    kind[p] = hit ? 1 : 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) { rgb[3 * p + d] = c[d]; nrm[3 * p + d] = m[d]; if (l) lit[3 * p + d] = l[d]; }
}

template <typename IDX>
__global__ __launch_bounds__(256) void k_rs_shade(const double* __restrict__ verts, int nv, const IDX* __restrict__ tris, long long nt,
                                                  const int* __restrict__ face, const float* __restrict__ bary, long long n,
                                                  const float* __restrict__ colors, const float* __restrict__ normals, unsigned char* __restrict__ kind,
                                                  float* __restrict__ rgb, float* __restrict__ nrm) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int idx[3];
    float c[3] = {0.f, 0.f, 0.f}, m[3] = {0.f, 0.f, 0.f};
    const bool hit = rs_hit(tris, nt, nv, face[p], idx);
    if (hit) {
        double b[3];
        rs_bary(bary, p, b);
#pragma unroll
        for (int d = 0; d < 3; ++d)
            c[d] = colors ? rs_interpolate(b, (double)colors[3 * (long long)idx[0] + d], (double)colors[3 * (long long)idx[1] + d], (double)colors[3 * (long long)idx[2] + d]) : 0.5f;
        if (normals) {
#pragma unroll
            for (int d = 0; d < 3; ++d)
                m[d] = rs_interpolate(b, (double)normals[3 * (long long)idx[0] + d], (double)normals[3 * (long long)idx[1] + d], (double)normals[3 * (long long)idx[2] + d]);
        } else rs_flat_normal_f32(verts, idx, m);
    }
    rs_store(p, hit, c, m, nullptr, kind, rgb, nrm, nullptr);
}

// the textured asset's shading; counters: bad_uv, flat_frame, back_lit (zeroed by the entry)
template <typename IDX>
__global__ __launch_bounds__(256) void k_rs_shade_tex(const double* __restrict__ verts, int nv, const IDX* __restrict__ tris, long long nt,
                                                      const int* __restrict__ face, const float* __restrict__ bary, long long n, const float* __restrict__ uv,
                                                      const uint8_t* __restrict__ image, const uint8_t* __restrict__ nimage, int Ht, int Wt,
                                                      const float* __restrict__ normals, const float* __restrict__ tangents, RsCamera cam, double ambient,
                                                      unsigned char* __restrict__ kind, float* __restrict__ rgb, float* __restrict__ nrm, float* __restrict__ lit,
                                                      unsigned long long* __restrict__ counters) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad_uv = false, flat_frame = false, back_lit = false;
    if (p < n) {
        const int t = face[p];
        int idx[3];
        float c[3] = {0.f, 0.f, 0.f}, m[3] = {0.f, 0.f, 0.f}, l[3] = {0.f, 0.f, 0.f};
        const bool hit = rs_hit(tris, nt, nv, t, idx);
        if (hit) {
            double b[3], u, v;
            rs_bary(bary, p, b);
            const bool good = rt_uv(b, uv + 6 * (long long)t, u, v);
            bad_uv = !good;
            RtTaps taps;
            if (good) {
                double value[3];
                rt_taps(u, v, Ht, Wt, taps);
                rt_fetch(image, Wt, taps, value);
#pragma unroll
                for (int d = 0; d < 3; ++d) c[d] = rt_albedo(value[d]);
            }
            if (nimage) {
                const float* N = normals + 9 * (long long)t;
                if (good) {
                    double s[3];
                    rt_fetch(nimage, Wt, taps, s);
                    flat_frame = !rt_normal(s, N, tangents + 12 * (long long)t, m);
                } else {
#pragma unroll
                    for (int d = 0; d < 3; ++d) m[d] = N[d];
                }
            } else rs_flat_normal_f32(verts, idx, m);
            if (good) {
                const double factor = rt_shade(cam, (int)(p % cam.W), (int)(p / cam.W), m, ambient, back_lit);
#pragma unroll
                for (int d = 0; d < 3; ++d) l[d] = rt_lit(c[d], factor);
            }
        }
        rs_store(p, hit, c, m, l, kind, rgb, nrm, lit);
    }
    wave_count(bad_uv, counters);
    wave_count(flat_frame, counters + 1);
    wave_count(back_lit, counters + 2);
}

struct RsCarve {
    RsTotals* tot;
    RsFace* faces;
    int *tile_count, *tile_start, *cursor, *block;
    long long n_tiles;
    unsigned nb;
};

static bool rs_image_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W < (1ll << 31); }
static bool rs_sizes_ok(long long nv, long long nt, int H, int W) { return mesh_sizes_ok(nv, nt) && rs_image_ok(H, W); }
#define RS_REQUIRE_SIZES(unit, nv, nt) O2345_REQUIRE(mesh_sizes_ok(nv, nt), unit ": bad sizes (nv must stay below 2^30 and 3 * nt below 2^31)")
// the one walk through the workspace: carves it, or sizes it when ws is null; returns its size
static size_t rs_carve(void* ws, long long nv, long long nt, int H, int W, RsCarve& c) {
    (void)nv;                                                        // nothing is kept per vertex
    c.n_tiles = (long long)((W + RS_TILE - 1) / RS_TILE) * ((H + RS_TILE - 1) / RS_TILE);
    c.nb = cdiv(c.n_tiles, SCAN_TILE);
    Carver w(ws);
    c.tot = w.take_bytes<RsTotals>(128);
    c.faces = w.take<RsFace>(nt);
    for (int** a : {&c.tile_count, &c.tile_start, &c.cursor}) *a = w.take<int>(c.n_tiles);
    c.block = w.take<int>(c.nb);
    return w.bytes();
}

// the checked camera of an entry from K [9] and c2w [12] on the host, both row-major; false: refused (the error is set)
static bool rs_entry_camera(const char* unit, const float* K, const float* c2w, int H, int W, double near, int cull, int ray_depth, RsCamera& cam) {
    if (!K || !c2w) { set_error("%s: null pointer", unit); return false; }
    if (!rs_image_ok(H, W)) { set_error("%s: bad image size %d x %d", unit, H, W); return false; }
    if (!(near > 0.0 && near <= DBL_MAX)) { set_error("%s: near must be finite and > 0, got %g", unit, near); return false; }
    if (cull < 0 || cull > 2) { set_error("%s: cull is 0 (none), 1 (back faces) or 2 (front faces), got %d", unit, cull); return false; }
    if (!(K[1] == 0.f && K[3] == 0.f && K[6] == 0.f && K[7] == 0.f && K[8] == 1.f)) {
        set_error("%s: a pinhole camera without skew is [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] with fx, fy != 0", unit); return false;
    }
    const float k4[4] = {K[0], K[4], K[2], K[5]}, m[12] = {c2w[0], c2w[1], c2w[2], c2w[3], c2w[4], c2w[5], c2w[6], c2w[7], c2w[8], c2w[9], c2w[10], c2w[11]};
    switch (rs_camera(k4, m, H, W, near, cull, ray_depth, cam)) {
        case 0: return true;
        case 1: set_error("%s: K and c2w must be finite", unit); return false;
        case 2: set_error("%s: fx and fy must be > 0", unit); return false;
        default: set_error("%s: the 3 x 3 of c2w must be a rotation (|R^T R - I| <= 1e-5 in every entry)", unit); return false;
    }
}

}  // namespace o2345

using namespace o2345;

extern "C" {

size_t o2345_mesh_raster_workspace_bytes(long long nv, long long nt, int H, int W) {
    if (!rs_sizes_ok(nv, nt, H, W)) return 0;
    RsCarve c;
    return rs_carve(nullptr, nv, nt, H, W, c);
}

// Pass 1: the faces to the screen, their classes, the tile counts and the starts of the tile lists, all inside the workspace; the counts go to `counts`
// on the DEVICE (the covered pixels are pass 2's).  No host synchronisation.
int o2345_mesh_raster_count(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, const float* K_host,
                            const float* c2w_host, int H, int W, double near, int cull, void* workspace, size_t workspace_bytes, long long* counts, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_raster_count", index_bytes);
    RS_REQUIRE_SIZES("mesh_raster_count", nv, nt);
    RsCamera cam;
    if (!rs_entry_camera("mesh_raster_count", K_host, c2w_host, H, W, near, cull, 0, cam)) return -1;
    O2345_REQUIRE(counts && (nt == 0 || tris) && (nv == 0 || verts), "mesh_raster_count: null pointer");
    O2345_REQUIRE(((uintptr_t)counts & 7) == 0, "mesh_raster_count: counts must be 8-byte aligned");
    O2345_REQUIRE_WORKSPACE("mesh_raster_count", workspace, workspace_bytes, o2345_mesh_raster_workspace_bytes(nv, nt, H, W));
    RsCarve c;
    (void)rs_carve(workspace, nv, nt, H, W, c);
    hipStream_t s = (hipStream_t)stream;
    O2345_HIP(hipMemsetAsync(c.tot, 0, 128, s));
    O2345_HIP(hipMemsetAsync(c.tile_count, 0, (size_t)c.n_tiles * sizeof(int), s));
    if (nt > 0)
        with_index_type(index_bytes, tris, [&](auto* t) {
            hipLaunchKernelGGL((k_rs_setup<index_type<decltype(t)>, false>), dim3(cdiv(nt, 256)), dim3(256), 0, s, verts, (int)nv, t, nt, cam, c.faces, c.tile_count,
                               (const int*)nullptr, (int*)nullptr, (int*)nullptr, 0ll, c.tot);
        });
    exclusive_scan<SCAN_ITEMS>(c.tile_count, c.n_tiles, c.nb, c.block, c.tile_start, nullptr, &c.tot->scan_total, s);
    hipLaunchKernelGGL(k_rs_counts, dim3(1), dim3(64), 0, s, c.tot, counts, 0);
    return check_launch("mesh_raster_count");
}

// Pass 2: the tile lists (lists: device int32 [n_pairs], n_pairs as counted) and the image, from the workspace of pass 1 (same sizes and camera,
// untouched in between); counts[O2345_RASTER_PIXELS] is written
int o2345_mesh_raster_emit(long long nv, long long nt, const float* K_host, const float* c2w_host, int H, int W, double near, int cull, int ray_depth,
                           void* workspace, size_t workspace_bytes, long long n_pairs, int* lists, int* face, float* depth, float* bary, long long* counts,
                           void* stream) {
    RS_REQUIRE_SIZES("mesh_raster_emit", nv, nt);
    RsCamera cam;
    if (!rs_entry_camera("mesh_raster_emit", K_host, c2w_host, H, W, near, cull, ray_depth, cam)) return -1;
    O2345_REQUIRE(n_pairs >= 0 && n_pairs < RS_MAX_PAIRS && (nt > 0 || n_pairs == 0), "mesh_raster_emit: bad pair count %lld (the limit is 2^31 - 1)", n_pairs);
    O2345_REQUIRE(face && depth && bary && counts && (n_pairs == 0 || lists), "mesh_raster_emit: null pointer");
    O2345_REQUIRE(((uintptr_t)counts & 7) == 0, "mesh_raster_emit: counts must be 8-byte aligned");
    O2345_REQUIRE_WORKSPACE("mesh_raster_emit", workspace, workspace_bytes, o2345_mesh_raster_workspace_bytes(nv, nt, H, W));
    RsCarve c;
    (void)rs_carve(workspace, nv, nt, H, W, c);
    hipStream_t s = (hipStream_t)stream;
    O2345_HIP(hipMemsetAsync(c.cursor, 0, (size_t)c.n_tiles * sizeof(int), s));      // a second emit starts over
    O2345_HIP(hipMemsetAsync(&c.tot->pixels, 0, sizeof(unsigned long long), s));
    if (nt > 0 && n_pairs > 0)
        hipLaunchKernelGGL((k_rs_setup<int, true>), dim3(cdiv(nt, 256)), dim3(256), 0, s, (const double*)nullptr, (int)nv, (const int*)nullptr, nt, cam, c.faces,
                           (int*)nullptr, c.tile_start, c.cursor, lists, n_pairs, c.tot);
    hipLaunchKernelGGL(k_rs_tiles, dim3((unsigned)c.n_tiles), dim3(64), 0, s, c.faces, nt, c.tile_start, c.tile_count, lists, n_pairs, cam, face, depth, bary, c.tot);
    hipLaunchKernelGGL(k_rs_counts, dim3(1), dim3(64), 0, s, c.tot, counts, 1);
    return check_launch("mesh_raster_emit");
}

// kind uint8 [H W], rgb and nrm float32 [H W,3] from face and bary: the inputs of o2345_surface_pack
int o2345_mesh_raster_shade(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, const int* face, const float* bary, int H, int W,
                            const float* colors_or_null, const float* normals_or_null, uint8_t* kind, float* rgb, float* nrm, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_raster_shade", index_bytes);
    RS_REQUIRE_SIZES("mesh_raster_shade", nv, nt);
    O2345_REQUIRE(rs_image_ok(H, W), "mesh_raster_shade: bad image size %d x %d", H, W);
    O2345_REQUIRE(face && bary && kind && rgb && nrm && (nt == 0 || tris) && (nv == 0 || verts), "mesh_raster_shade: null pointer");
    const long long n = (long long)H * W;
    with_index_type(index_bytes, tris, [&](auto* t) {
        hipLaunchKernelGGL(k_rs_shade<index_type<decltype(t)>>, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, verts, (int)nv, t, nt, face, bary, n,
                           colors_or_null, normals_or_null, kind, rgb, nrm);
    });
    return check_launch("mesh_raster_shade");
}

// The textured asset's shading from face and bary (include/o2345.h has the definition): kind, rgb (the atlas's albedo), nrm, lit and the counters.
// No host synchronisation.
int o2345_mesh_raster_shade_textured(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, const int* face, const float* bary,
                                     const float* uv, const uint8_t* image, int tex_h, int tex_w, const uint8_t* normal_image_or_null,
                                     const float* normals_or_null, const float* tangents_or_null, const float* K_host, const float* c2w_host, int H, int W,
                                     float ambient, uint8_t* kind, float* rgb, float* nrm, float* lit, long long* counters, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_raster_shade_textured", index_bytes);
    RS_REQUIRE_SIZES("mesh_raster_shade_textured", nv, nt);
    RsCamera cam;
    if (!rs_entry_camera("mesh_raster_shade_textured", K_host, c2w_host, H, W, 1.0, 0, 0, cam)) return -1;
    O2345_REQUIRE(tex_h >= 1 && tex_w >= 1 && tex_h <= RT_MAX_SIDE && tex_w <= RT_MAX_SIDE && (long long)tex_h * tex_w < (1ll << 31),
                  "mesh_raster_shade_textured: bad atlas size %d x %d (a side is limited to %d)", tex_w, tex_h, RT_MAX_SIDE);
    O2345_REQUIRE(!normal_image_or_null == !normals_or_null && !normals_or_null == !tangents_or_null,
                  "mesh_raster_shade_textured: a normal map is the normal image, the normals and the tangents together");
    O2345_REQUIRE(ambient >= 0.f && ambient <= 1.f, "mesh_raster_shade_textured: ambient must be in [0, 1], got %g", (double)ambient);
    O2345_REQUIRE(face && bary && image && kind && rgb && nrm && lit && counters && (nt == 0 || (tris && uv)) && (nv == 0 || verts),
                  "mesh_raster_shade_textured: null pointer");
    O2345_REQUIRE(((uintptr_t)counters & 7) == 0 && ((uintptr_t)image & 3) == 0 && ((uintptr_t)normal_image_or_null & 3) == 0,
                  "mesh_raster_shade_textured: counters must be 8-byte aligned and the images 4-byte aligned");
    const long long n = (long long)H * W;
    hipStream_t s = (hipStream_t)stream;
    O2345_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(long long), s));
    with_index_type(index_bytes, tris, [&](auto* t) {
        hipLaunchKernelGGL(k_rs_shade_tex<index_type<decltype(t)>>, dim3(cdiv(n, 256)), dim3(256), 0, s, verts, (int)nv, t, nt, face, bary, n, uv, image,
                           normal_image_or_null, tex_h, tex_w, normals_or_null, tangents_or_null, cam, (double)ambient, kind, rgb, nrm, lit,
                           (unsigned long long*)counters);
    });
    return check_launch("mesh_raster_shade_textured");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_mesh_raster() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)k_rs_counts);
}
}  // namespace o2345
