// Texture atlas of the exported mesh on the device: the surface point of every texel (k_tex_points), the image from the texel colours (k_tex_pack) and
// the unwelded, uv-carrying vertices (k_tex_corners).  The colours in between come from the library's own network kernels over the point list.  Equal to
// the host twins (mesh_io.texture_points / pack_texture / texture_corners) to the last bit: everything here is fp64, one operation at a time, in a
// defined order, or integer.
//
// Layout (c = texel, the edge of a cell in texels, 4 .. 64; nt triangles)
//   cells      triangles 2k and 2k + 1, in face order, share square cell k; cells = ceil(nt / 2), G = ceil(sqrt(cells)); cell k sits at column k mod G,
//              row k div G; the image is W = G c wide and H = ceil(cells / G) c high.  W, H <= 16384 and cells c^2 < 2^31.
//   in a cell  local texel (i, j) has its centre at (i + 0.5, j + 0.5).  Triangle A = 2k has its corners at local uv (0.5, 0.5), (c - 1.5, 0.5),
//              (0.5, c - 1.5) and owns the texels with i + j <= c - 1; triangle B = min(2k + 1, nt - 1) has them at (c - 0.5, c - 0.5), (2.5, c - 0.5),
//              (c - 0.5, 2.5) and owns those with i + j >= c.  For an odd nt the B half of the last cell repeats the last triangle.
//   why        a bilinear fetch (texel centres at + 0.5, clamp to edge, no mipmaps) anywhere in a triangle, edges and corners included, reads only texels
//              its triangle owns: for A the centre-relative coordinates x, y >= 0 have x + y <= c - 2, so ceil(x) + ceil(y) <= c - 1 wherever the weight
//              is not zero; for B x, y <= c - 1 and x + y >= c + 1, so floor(x) + floor(y) >= c.  Nothing bleeds, no dilation pass is needed.
//   texel      barycentric weights of the centre with respect to the owner's uv corners -- A: w1 = i / (c - 2), w2 = j / (c - 2); B: w1 = (c - 1 - i) /
//              (c - 3), w2 = (c - 1 - j) / (c - 3); w0 = (1 - w1) - w2 -- NOT clamped: gutter texels extrapolate, which makes the bilinear fetch of a
//              function linear over the triangle's plane exact.  p = (w0 P0 + w1 P1) + w2 P2 on the index-space vertices, each coordinate clamped to
//              [0, R - 1]; world point float32(p / (R - 1) * ext + bmin), bmin / bmax the float32 bounds widened, ext = bmax - bmin: mesh_project's.
//   order      texel points and colours are cell-major: entry k c^2 + j c + i.  Exactly cells c^2 entries, no compaction.
//   corners    triangle t = (a, b, c) gives unwelded vertices 3t, 3t + 1, 3t + 2 = c, b, a (the asset frame's reversed winding); uv = ((cell_x c + u_local)
//              / W, (cell_y c + v_local) / H) in fp64, rounded once; position and normal are the welded export's for that vertex (mesh_math.h).
// Bad input never faults: a triangle index outside [0, nv) is read as vertex 0, and it and a non-finite coordinate are counted once per triangle in two
// integer counters that the caller raises on.  No other atomics.  Nothing here synchronises with the host.
//
// Normal map (opt-in): k_tex_frames gives every triangle of the file a tangent frame from the float32 buffers k_tex_corners wrote, k_tex_normal_pack turns
// the SDF gradients at the texel points -- which the colour network needed anyway -- into the RGBA8 tangent-space image.  The definition is in
// include/o2345.h, the arithmetic in mesh_normalmap_math.h, the host twins are mesh_io.texture_frames / pack_normal_map.
#include "mesh_math.h"
#include "mesh_normalmap_math.h"

namespace o2345 {

struct TexLayout {
    int c, G, W, H;
    long long cells, texels;
};

// host: the layout, or false for what the definition refuses
static bool tex_layout(long long nt, int c, TexLayout& L) {
    if (nt < 1 || nt >= (1ll << 40) || c < 4 || c > 64) return false;
    const long long cells = (nt + 1) / 2;
    long long g = (long long)sqrt((double)cells);
    while (g * g < cells) ++g;
    while (g > 1 && (g - 1) * (g - 1) >= cells) --g;
    const long long rows = (cells + g - 1) / g;
    if (g * c > 16384 || rows * c > 16384 || cells * c * c >= (1ll << 31)) return false;
    L.c = c; L.G = (int)g; L.W = (int)(g * c); L.H = (int)(rows * c); L.cells = cells; L.texels = cells * c * c;
    return true;
}

#define TEX_REQUIRE_LAYOUT(unit, nt, texel, L) \
    O2345_REQUIRE(tex_layout(nt, texel, L), unit ": bad layout (nt = %lld >= 1, texel = %d in [4, 64], sides <= 16384, texels < 2^31)", nt, texel)
// the owner of a texel of cell k: the B half (i + j >= c) is triangle 2k + 1's where there is one
__device__ __forceinline__ long long tex_owner(long long k, bool isB, long long nt) { return isB && 2 * k + 1 < nt ? 2 * k + 1 : 2 * k; }

// the walk from image texel e (raster order) to its cell k, cell-major slot s, owner t and local (i, j); used: the cell holds triangles
struct TexWalk { bool used; long long k, s, t; int i, j; };
__device__ __forceinline__ TexWalk tex_walk(const TexLayout& L, long long e, long long nt) {
    const int y = (int)(e / L.W), x = (int)(e - (long long)y * L.W), cx = x / L.c, cy = y / L.c, i = x - cx * L.c, j = y - cy * L.c;
    const long long k = (long long)cy * L.G + cx;
    return {k < L.cells, k, k * L.c * L.c + (long long)j * L.c + i, tex_owner(k, i + j >= L.c, nt), i, j};
}

// thread per texel of a used cell, cell-major
template <typename IDX>
__global__ __launch_bounds__(256) void k_tex_points(const double* __restrict__ verts, long long nv, const IDX* __restrict__ tris, long long nt, int c,
                                                    long long texels, IndexFrame f, double* __restrict__ pidx, float* __restrict__ pworld,
                                                    O2345TextureStats* __restrict__ st) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false, nonfinite = false;
    if (e < texels) {
        const int cc = c * c;
        const long long k = e / cc;
        const int r = (int)(e - k * cc), j = r / c, i = r - j * c;
        const bool isB = i + j >= c;
        const long long t = tex_owner(k, isB, nt);
        const bool counts = isB ? (t != 2 * k && i == c - 1 && j == c - 1) : (i == 0 && j == 0);  // one texel speaks for its triangle
        double w1, w2;
        if (isB) { w1 = __ddiv_rn((double)(c - 1 - i), (double)(c - 3)); w2 = __ddiv_rn((double)(c - 1 - j), (double)(c - 3)); }
        else { w1 = __ddiv_rn((double)i, (double)(c - 2)); w2 = __ddiv_rn((double)j, (double)(c - 2)); }
        const double w0 = __dsub_rn(__dsub_rn(1.0, w1), w2);
        double P[3][3];
        bool tb = false, tn = false;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            long long v = (long long)tris[3 * t + q];
            if (v < 0 || v >= nv) { tb = true; v = 0; }
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                P[q][d] = verts[3 * v + d];
                tn |= !finite(P[q][d]);
            }
        }
        bad = counts && tb;
        nonfinite = counts && tn && !tb;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            double y = __dadd_rn(__dadd_rn(__dmul_rn(w0, P[0][d]), __dmul_rn(w1, P[1][d])), __dmul_rn(w2, P[2][d]));
            if (y < 0.0) y = 0.0; else if (y > f.rm1) y = f.rm1;
            pidx[3 * e + d] = y;
            pworld[3 * e + d] = index_to_world_f32(y, f, d);
        }
    }
    wave_count(bad, &st->n_bad);
    wave_count(nonfinite, &st->n_nonfinite);
}

// thread per image texel, raster order: one aligned uchar4 store each
__global__ __launch_bounds__(256) void k_tex_pack(const float* __restrict__ rgb, TexLayout L, uchar4* __restrict__ image) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)L.W * L.H) return;
    const TexWalk w = tex_walk(L, e, 0);                                 // the owner is not read
    uchar4 o = make_uchar4(0, 0, 0, 0);
    if (w.used) o = make_uchar4(mesh_colour_u8(rgb[3 * w.s]), mesh_colour_u8(rgb[3 * w.s + 1]), mesh_colour_u8(rgb[3 * w.s + 2]), 255);
    image[e] = o;
}

// thread per unwelded vertex q = 3t + d, which is corner 2 - d of triangle t; per-block min / max of the float32 positions -> partials[block][6]
template <typename IDX>
__global__ __launch_bounds__(256) void k_tex_corners(const double* __restrict__ verts, long long nv, const IDX* __restrict__ tris, long long n3, TexLayout L,
                                                     MeshXform x, const float* __restrict__ grad, float* __restrict__ pos, float* __restrict__ uv,
                                                     float* __restrict__ nrm, uint32_t* __restrict__ idx, float* __restrict__ partials) {
    __shared__ float red[24];
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (q < n3) {
        const long long t = q / 3;
        const int s = 2 - (int)(q - 3 * t);
        long long v = (long long)tris[3 * t + s];
        if (v < 0 || v >= nv) v = 0;                                    // counted by k_tex_points; never dereferenced
        float p[3];
        mesh_vertex_f32(verts, v, x, p);
        const float a[3] = {p[0], p[2], p[1]};
#pragma unroll
        for (int d = 0; d < 3; ++d) { pos[3 * q + d] = a[d]; mn[d] = a[d]; mx[d] = a[d]; }
        const long long k = t >> 1;
        const int cx = (int)(k % L.G), cy = (int)(k / L.G), c = L.c;
        double ul, vl;
        if (t & 1) { ul = s == 1 ? 2.5 : (double)c - 0.5; vl = s == 2 ? 2.5 : (double)c - 0.5; }
        else { ul = s == 1 ? (double)c - 1.5 : 0.5; vl = s == 2 ? (double)c - 1.5 : 0.5; }
        uv[2 * q] = (float)__ddiv_rn(__dadd_rn((double)(cx * c), ul), (double)L.W);
        uv[2 * q + 1] = (float)__ddiv_rn(__dadd_rn((double)(cy * c), vl), (double)L.H);
        if (grad) mesh_normal_f32(grad, v, x, nrm + 3 * q);
        idx[q] = (uint32_t)q;
    }
    float out[6];
    block_minmax(mn, mx, red, out);
    if (threadIdx.x < 6) partials[(long long)blockIdx.x * 6 + threadIdx.x] = out[threadIdx.x];
}

// Tangent-space normal map (mesh_normalmap_math.h has the arithmetic; mesh_io.texture_frames / pack_normal_map are the host twins).
// thread per unwelded vertex q = 3t + d: every corner of a triangle computes, and stores, its triangle's frame; corner 0 speaks for it in the count
__global__ __launch_bounds__(256) void k_tex_frames(const float* __restrict__ pos, const float* __restrict__ uv, long long n3, float* __restrict__ nrm,
                                                    float4* __restrict__ tan, unsigned long long* __restrict__ counters) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    bool degenerate = false;
    if (q < n3) {
        const long long t = q / 3;
        float N[3], T[4];
        const bool ok = nm_frame(pos + 9 * t, uv + 6 * t, N, T);
        degenerate = !ok && q == 3 * t;
        nrm[3 * q] = N[0]; nrm[3 * q + 1] = N[1]; nrm[3 * q + 2] = N[2];
        tan[q] = make_float4(T[0], T[1], T[2], T[3]);
    }
    wave_count(degenerate, counters);
}

// thread per image texel, raster order: one aligned uchar4 store each
__global__ __launch_bounds__(256) void k_tex_normal_pack(const float* __restrict__ grad, const float* __restrict__ rotation, const float* __restrict__ nrm,
                                                         const float* __restrict__ tan, long long nt, TexLayout L, uchar4* __restrict__ image,
                                                         unsigned long long* __restrict__ counters) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    int flags = 0;
    if (e < (long long)L.W * L.H) {
        const TexWalk w = tex_walk(L, e, nt);
        uint8_t o[4] = {128, 128, 255, 255};
        if (w.used) flags = nm_texel(grad + 3 * w.s, rotation, nrm + 9 * w.t, tan + 12 * w.t, o);
        image[e] = make_uchar4(o[0], o[1], o[2], o[3]);
    }
    wave_count((flags & NM_BAD_GRADIENT) != 0, counters + 1);
    wave_count((flags & NM_BACK_FACING) != 0, counters + 2);
}

}  // namespace o2345

using namespace o2345;

extern "C" {

size_t o2345_mesh_texture_texels(long long nt, int texel, int* width_host, int* height_host) {
    TexLayout L;
    if (!tex_layout(nt, texel, L)) return 0;
    if (width_host) *width_host = L.W;
    if (height_host) *height_host = L.H;
    return (size_t)L.texels;
}

int o2345_mesh_texture_points(const double* verts, long long nv, const void* tris, int index_bytes, long long nt, int texel, int grid_R,
                              const float* bound_min, const float* bound_max, double* points_idx, float* points_world, O2345TextureStats* stats, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_texture_points", index_bytes);
    TexLayout L;
    TEX_REQUIRE_LAYOUT("mesh_texture_points", nt, texel, L);
    O2345_REQUIRE(nv >= 1 && nv < (1ll << 30), "mesh_texture_points: bad size (nv must be in [1, 2^30))");
    O2345_REQUIRE(grid_R >= 2, "mesh_texture_points: bad resolution %d", grid_R);
    O2345_REQUIRE(verts && tris && bound_min && bound_max && points_idx && points_world && stats, "mesh_texture_points: null pointer");
    O2345_REQUIRE(((uintptr_t)stats & 7) == 0, "mesh_texture_points: stats must be 8-byte aligned");
    IndexFrame f;
    if (!index_frame("mesh_texture_points", grid_R, bound_min, bound_max, f)) return -1;
    hipStream_t s = (hipStream_t)stream;
    O2345_HIP(hipMemsetAsync(stats, 0, sizeof *stats, s));
    const dim3 grid(cdiv(L.texels, 256));
    with_index_type(index_bytes, tris, [&](auto* t) {
        hipLaunchKernelGGL(k_tex_points<index_type<decltype(t)>>, grid, dim3(256), 0, s, verts, nv, t, nt, L.c, L.texels, f, points_idx, points_world, stats);
    });
    return check_launch("mesh_texture_points");
}

int o2345_mesh_texture_pack(const float* rgb, long long nt, int texel, uint8_t* image, void* stream) {
    TexLayout L;
    TEX_REQUIRE_LAYOUT("mesh_texture_pack", nt, texel, L);
    O2345_REQUIRE(rgb && image, "mesh_texture_pack: null pointer");
    O2345_REQUIRE(((uintptr_t)image & 3) == 0, "mesh_texture_pack: image must be 4-byte aligned");
    hipLaunchKernelGGL(k_tex_pack, dim3(cdiv((long long)L.W * L.H, 256)), dim3(256), 0, (hipStream_t)stream, rgb, L, (uchar4*)image);
    return check_launch("mesh_texture_pack");
}

int o2345_mesh_texture_corners(const double* verts, long long nv, const void* tris, int index_bytes, long long nt, int texel, int grid_R,
                               const float* bound_min, const float* bound_max, const float* scale_mat, const float* trans_mat, const float* grad,
                               float* positions, float* uv, float* normals, uint32_t* indices, float* bounds, void* workspace, size_t workspace_bytes,
                               void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_texture_corners", index_bytes);
    TexLayout L;
    TEX_REQUIRE_LAYOUT("mesh_texture_corners", nt, texel, L);
    O2345_REQUIRE(nv >= 1 && nv < (1ll << 30), "mesh_texture_corners: bad size (nv must be in [1, 2^30))");
    O2345_REQUIRE(bound_min && bound_max && grid_R >= 2, "mesh_texture_corners: bad bounds / resolution");
    O2345_REQUIRE(verts && tris && positions && uv && indices && bounds && workspace && (!grad || normals), "mesh_texture_corners: null pointer");
    const long long n3 = 3 * nt;
    O2345_REQUIRE(workspace_bytes >= o2345_mesh_bounds_workspace_bytes(n3), "mesh_texture_corners: workspace of %zu bytes, need %zu", workspace_bytes,
                  o2345_mesh_bounds_workspace_bytes(n3));
    O2345_REQUIRE(((uintptr_t)workspace & 3) == 0, "mesh_texture_corners: workspace must be 4-byte aligned");
    const MeshXform x = mesh_xform(grid_R, bound_min, bound_max, scale_mat, trans_mat);
    const unsigned nb = cdiv(n3, 256);
    hipStream_t s = (hipStream_t)stream;
    with_index_type(index_bytes, tris, [&](auto* t) {
        hipLaunchKernelGGL(k_tex_corners<index_type<decltype(t)>>, dim3(nb), dim3(256), 0, s, verts, nv, t, n3, L, x, grad, positions, uv, normals, indices, (float*)workspace);
    });
    mesh_bounds_finish((const float*)workspace, (long long)nb, bounds, s);
    return check_launch("mesh_texture_corners");
}

int o2345_mesh_texture_frames(const float* positions, const float* uv, long long nt, float* normals, float* tangents, long long* counters, void* stream) {
    O2345_REQUIRE(nt >= 1 && 3 * nt < (1ll << 31), "mesh_texture_frames: bad size (nt = %lld must be in [1, 2^31 / 3))", nt);
    O2345_REQUIRE(positions && uv && normals && tangents && counters, "mesh_texture_frames: null pointer");
    O2345_REQUIRE(((uintptr_t)tangents & 15) == 0, "mesh_texture_frames: tangents must be 16-byte aligned");
    O2345_REQUIRE(((uintptr_t)counters & 7) == 0, "mesh_texture_frames: counters must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    O2345_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(long long), s));
    hipLaunchKernelGGL(k_tex_frames, dim3(cdiv(3 * nt, 256)), dim3(256), 0, s, positions, uv, 3 * nt, normals, (float4*)tangents, (unsigned long long*)counters);
    return check_launch("mesh_texture_frames");
}

int o2345_mesh_texture_normal_pack(const float* grad, const float* rotation, const float* normals, const float* tangents, long long nt, int texel,
                                   uint8_t* image, long long* counters, void* stream) {
    TexLayout L;
    TEX_REQUIRE_LAYOUT("mesh_texture_normal_pack", nt, texel, L);
    O2345_REQUIRE(grad && normals && tangents && image && counters, "mesh_texture_normal_pack: null pointer");
    O2345_REQUIRE(((uintptr_t)image & 3) == 0, "mesh_texture_normal_pack: image must be 4-byte aligned");
    O2345_REQUIRE(((uintptr_t)counters & 7) == 0, "mesh_texture_normal_pack: counters must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    O2345_HIP(hipMemsetAsync(counters + 1, 0, 3 * sizeof(long long), s));                 // entry 0 is the frames call's
    hipLaunchKernelGGL(k_tex_normal_pack, dim3(cdiv((long long)L.W * L.H, 256)), dim3(256), 0, s, grad, rotation, normals, tangents, nt, L, (uchar4*)image,
                       (unsigned long long*)counters);
    return check_launch("mesh_texture_normal_pack");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_mesh_texture() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)k_tex_pack);
}
}  // namespace o2345
