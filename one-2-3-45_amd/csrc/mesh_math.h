// Per-element mesh arithmetic shared by the serialisation kernels (mesh_pack.hip: PLY records; mesh_export.hip: GLB buffers and OBJ text) and by
// their host-side packers: the marching-cubes index -> output frame transform, the colour quantisation, and the fixed-width decimal fields of the
// OBJ records.  One definition each, so that a PLY, a GLB and an OBJ of one mesh carry the same float32 positions and the same uint8 colours.  Also the
// index -> world frame of the units that evaluate the networks at mesh points (IndexFrame: mesh_project.hip, mesh_texture.hip).
#pragma once
#include "mesh_common.h"
#include <math.h>

namespace o2345 {

// The marching-cubes index -> world frame of the units that hand points to the network kernels (mesh_project.hip, mesh_texture.hip): the float32 bounds
// widened to fp64 and subtracted there.  (MeshXform below subtracts in fp32, as the reference's export does, and carries the asset transforms.)
struct IndexFrame {
    double rm1;                                       // R - 1
    double bmin[3], bext[3];                          // bound_min, bound_max - bound_min
};

// host: the frame from the C ABI's host arrays; false with the unit's error set
inline bool index_frame(const char* unit, int grid_R, const float* bound_min, const float* bound_max, IndexFrame& f) {
    f.rm1 = (double)grid_R - 1.0;
    for (int k = 0; k < 3; ++k) {
        f.bmin[k] = (double)bound_min[k];
        f.bext[k] = (double)bound_max[k] - (double)bound_min[k];
        if (!(f.bext[k] > 0.0 && finite(f.bext[k]) && finite(f.bmin[k]))) {
            set_error("%s: bound_max must be above bound_min on every axis, both finite", unit);
            return false;
        }
    }
    return true;
}

// float32(x / (R - 1) * ext_k + bmin_k) for axis k, one rounding per operation: for the bounds (-1, 1) the pipeline's verts_idx / (R - 1) * 2 - 1 to the
// bit; and the three axes of a point
__device__ __forceinline__ float index_to_world_f32(double x, const IndexFrame& f, int k) {
    return (float)__dadd_rn(__dmul_rn(__ddiv_rn(x, f.rm1), f.bext[k]), f.bmin[k]);
}
__device__ __forceinline__ void index_to_world_f32(const double (&x)[3], const IndexFrame& f, float* __restrict__ out) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = index_to_world_f32(x[k], f, k);
}

struct MeshXform {
    double inv_rm1;            // 1 / (R - 1)   (the reference divides; kept as a division below)
    int R;
    double bmin[3], bext[3];   // bound_min, bound_max - bound_min
    int has_scale; double s, t[3];          // scale_mat[0,0], scale_mat[:3,3]
    int has_trans; double T[12];            // rows 0..2 of trans_mat (4x4, row-major)
};

// host: the kernel argument from the C ABI's host arrays (bound_min[3], bound_max[3], scale_mat / trans_mat 4x4 row-major fp32 or NULL)
inline MeshXform mesh_xform(int grid_R, const float* bound_min, const float* bound_max, const float* scale_mat, const float* trans_mat) {
    MeshXform x{};
    x.R = grid_R;
    for (int d = 0; d < 3; ++d) { x.bmin[d] = (double)bound_min[d]; x.bext[d] = (double)(bound_max[d] - bound_min[d]); }   // fp32 subtraction, as torch does
    x.has_scale = scale_mat != nullptr;
    if (scale_mat) { x.s = (double)scale_mat[0]; x.t[0] = (double)scale_mat[3]; x.t[1] = (double)scale_mat[7]; x.t[2] = (double)scale_mat[11]; }
    x.has_trans = trans_mat != nullptr;
    if (trans_mat) for (int k = 0; k < 12; ++k) x.T[k] = (double)trans_mat[k];
    return x;
}

// Index coordinates of vertex i -> the reference's export frame in fp64 (sparse_neus_renderer.py:936: v / (R - 1) * (bmax - bmin) + bmin;
// trainer_generic.py:1365-1372: * s + t, then trans @ [v, 1]), rounded to float32 once, at the end -- what trimesh's PLY exporter stores.
O2345_HD void mesh_vertex_f32(const double* __restrict__ vidx, long long i, const MeshXform& x, float f[3]) {
    double v[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        v[d] = vidx[3 * i + d] / (double)(x.R - 1) * x.bext[d] + x.bmin[d];        // sparse_neus_renderer.py:936
        if (x.has_scale) v[d] = v[d] * x.s + x.t[d];
    }
    if (x.has_trans) {
        double w[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) w[r] = ((x.T[4 * r] * v[0] + x.T[4 * r + 1] * v[1]) + x.T[4 * r + 2] * v[2]) + x.T[4 * r + 3];
        v[0] = w[0]; v[1] = w[1]; v[2] = w[2];
    }
    f[0] = (float)v[0]; f[1] = (float)v[1]; f[2] = (float)v[2];
}

// SDF gradient of vertex i -> unit normal of the asset frame: normalize(g) -> 3x3 of trans_mat -> renormalise, in fp64, y and z exchanged; scale_mat is
// a positive uniform scale and leaves a direction alone.  (0, 1, 0) for a zero or non-finite gradient.
O2345_HD void mesh_normal_f32(const float* __restrict__ grad, long long i, const MeshXform& x, float n[3]) {
    double g[3] = {(double)grad[3 * i], (double)grad[3 * i + 1], (double)grad[3 * i + 2]};
    double l = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    bool ok = l > 0.0 && l < (double)INFINITY;
    if (ok) {
        g[0] /= l; g[1] /= l; g[2] /= l;
        if (x.has_trans) {
            double w[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) w[r] = (x.T[4 * r] * g[0] + x.T[4 * r + 1] * g[1]) + x.T[4 * r + 2] * g[2];
            l = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
            ok = l > 0.0 && l < (double)INFINITY;
            g[0] = w[0] / l; g[1] = w[1] / l; g[2] = w[2] / l;
        }
    }
    n[0] = ok ? (float)g[0] : 0.f;
    n[1] = ok ? (float)g[2] : 1.f;
    n[2] = ok ? (float)g[1] : 0.f;
}

// n = g / l with l = sqrt((gx gx + gy gy) + gz gz) in fp64, the length mesh_normal_f32 takes -> true; a zero or non-finite length gives n = 0 and false
O2345_HD bool unit_normal(const double (&g)[3], double (&n)[3]) {
    const double l = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    const bool ok = l > 0.0 && l < (double)INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = ok ? g[k] / l : 0.0;
    return ok;
}

// np.array(color * 255, dtype=uint8) (trainer_generic.py:1377): truncation
O2345_HD uint8_t mesh_colour_u8(float c) { return (uint8_t)(int)(c * 255.f); }

// ---- per-axis bounds of float32 positions: stage one per block (block_minmax -> partials[block][6]), stage two in mesh_export.hip -----------------
// min / max of six per-thread values over a 256-thread block -> out[0..5] valid in threads 0..5 after the call (lds: 4 x 6 floats)
__device__ __forceinline__ void block_minmax(float mn[3], float mx[3], float* lds, float out[6]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            mn[d] = fminf(mn[d], __shfl_xor(mn[d], off));
            mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], off));
        }
    }
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { lds[w * 6 + d] = mn[d]; lds[w * 6 + 3 + d] = mx[d]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        float r = lds[k];
        for (int i = 1; i < 4; ++i) r = k < 3 ? fminf(r, lds[i * 6 + k]) : fmaxf(r, lds[i * 6 + k]);
        out[k] = r;
    }
}
// stage two (mesh_export.hip): ONE block folds nblocks x 6 partials -> bounds[0..2] = min, bounds[3..5] = max, queued on `stream`
void mesh_bounds_finish(const float* partials, long long nblocks, float* bounds, hipStream_t stream);

// ---- OBJ text fields ------------------------------------------------------------------------------------------------------------------------
// Every field is written right to left into exactly `width` bytes, whatever the value: a value that needs more room than the host planned for
// loses its leading characters, it never moves a neighbour.

// " %*.8f" of a float32 in `width` = 1 (space) + 1 (sign) + K + 1 + 8 bytes.  (double)|v| * 1e8 is exact (24-bit significand x 5^8 < 2^53), so rint
// (to nearest, ties to even) and integer digit extraction give printf's correctly rounded digits; the sign comes from the sign bit ("-0.00000000").
O2345_HD void obj_fixed8(uint8_t* dst, int width, float v) {
    int p = width - 1;
    if (!(fabsf(v) <= 3.4028234e38f)) {                  // printf's "nan" / "inf" / "-inf"
        const bool nan = v != v;
        dst[p--] = nan ? 'n' : 'f'; if (p >= 0) dst[p--] = nan ? 'a' : 'n'; if (p >= 0) dst[p--] = nan ? 'n' : 'i';
        if (!nan && v < 0.f && p >= 0) dst[p--] = '-';
        while (p >= 0) dst[p--] = ' ';
        return;
    }
    const double a = rint((double)fabsf(v) * 1e8);
    const unsigned long long q = a < 1.8e19 ? (unsigned long long)a : 0ull;
    unsigned frac = (unsigned)(q % 100000000ull);
    unsigned long long ip = q / 100000000ull;
    for (int k = 0; k < 8 && p >= 0; ++k) { dst[p--] = (uint8_t)('0' + frac % 10u); frac /= 10u; }
    if (p >= 0) dst[p--] = '.';
    do { if (p >= 0) dst[p--] = (uint8_t)('0' + (unsigned)(ip % 10ull)); ip /= 10ull; } while (ip);
    if (__builtin_signbit(v) && p >= 0) dst[p--] = '-';
    while (p >= 0) dst[p--] = ' ';
}

// "%*u" right-aligned in `width` bytes; returns the position left of the first digit
O2345_HD int obj_uint(uint8_t* dst, int p, unsigned v) {
    do { if (p >= 0) dst[p--] = (uint8_t)('0' + v % 10u); v /= 10u; } while (v);
    return p;
}

struct ObjLayout {
    int K;             // integer digits of a coordinate field
    int dn;            // decimal digits of the vertex count
    int colours, normals;
    int v_len, vn_len, f_len;
    int vt_len, ft_len;    // the textured file's "vt" record and its "f a/a b/b c/c" record over unwelded corners
};

O2345_HD int obj_digits(unsigned long long v) { int d = 1; while (v >= 10ull) { v /= 10ull; ++d; } return d; }

O2345_HD ObjLayout obj_layout(long long n, int K, int colours, int normals) {
    ObjLayout L;
    L.K = K; L.dn = obj_digits((unsigned long long)(n > 0 ? n : 0)); L.colours = colours; L.normals = normals;
    L.v_len = 1 + 3 * (K + 11) + (colours ? 33 : 0) + 1;
    L.vn_len = 2 + 3 * 12 + 1;
    L.f_len = 1 + 3 * (1 + (normals ? 2 * L.dn + 2 : L.dn)) + 1;
    L.vt_len = 2 + 2 * 11 + 1;
    L.ft_len = 1 + 3 * (1 + (normals ? 3 * L.dn + 2 : 2 * L.dn + 1)) + 1;
    return L;
}

// "v" + 3 coordinate fields [+ 3 colour fields from the 256 x 11-byte table " %.8f" % (c / 255)] + "\n"
O2345_HD void obj_vertex_record(uint8_t* dst, const ObjLayout& L, const float* pos, const uint8_t* rgba, const uint8_t* table) {
    dst[0] = 'v';
    const int w = L.K + 11;
#pragma unroll
    for (int d = 0; d < 3; ++d) obj_fixed8(dst + 1 + d * w, w, pos[d]);
    uint8_t* c = dst + 1 + 3 * w;
    if (L.colours) {
        for (int d = 0; d < 3; ++d, c += 11) {
            const uint8_t* t = table + 11 * (int)rgba[d];
            for (int k = 0; k < 11; ++k) c[k] = t[k];
        }
    }
    c[0] = '\n';
}

// "vn" + 3 x " %11.8f" + "\n"
O2345_HD void obj_normal_record(uint8_t* dst, const float* nrm) {
    dst[0] = 'v'; dst[1] = 'n';
#pragma unroll
    for (int d = 0; d < 3; ++d) obj_fixed8(dst + 2 + d * 12, 12, nrm[d]);
    dst[38] = '\n';
}

// "f" + 3 x " %*d" (1-based) + "\n", or 3 x " a//a" with each token right-aligned in 2 * dn + 2 bytes
O2345_HD void obj_face_record(uint8_t* dst, const ObjLayout& L, const uint32_t* idx) {
    dst[0] = 'f';
    const int w = 1 + (L.normals ? 2 * L.dn + 2 : L.dn);
    for (int d = 0; d < 3; ++d) {
        uint8_t* o = dst + 1 + d * w;
        const unsigned a = idx[d] + 1u;
        int p = obj_uint(o, w - 1, a);
        if (L.normals) {
            if (p >= 0) o[p--] = '/';
            if (p >= 0) o[p--] = '/';
            p = obj_uint(o, p, a);
        }
        while (p >= 0) o[p--] = ' ';
    }
    dst[1 + 3 * w] = '\n';
}

// "vt" + 2 x " %10.8f" + "\n": u, then float32(1 - v) -- the image's row 0 is its top, OBJ's v = 0 its bottom
O2345_HD void obj_texcoord_record(uint8_t* dst, const float* uv) {
    dst[0] = 'v'; dst[1] = 't';
    obj_fixed8(dst + 2, 11, uv[0]);
    obj_fixed8(dst + 13, 11, (float)(1.0 - (double)uv[1]));
    dst[24] = '\n';
}

// "f" + 3 x " a/a" (or " a/a/a" with normals) over the unwelded corners 3t + 1 .. 3t + 3 of triangle t, each token right-aligned in 2 dn + 1 (3 dn + 2) bytes
O2345_HD void obj_corner_face_record(uint8_t* dst, const ObjLayout& L, unsigned t) {
    dst[0] = 'f';
    const int w = 1 + (L.normals ? 3 * L.dn + 2 : 2 * L.dn + 1);
    for (int d = 0; d < 3; ++d) {
        uint8_t* o = dst + 1 + d * w;
        const unsigned a = 3u * t + (unsigned)d + 1u;
        int p = obj_uint(o, w - 1, a);
        for (int k = L.normals ? 2 : 1; k > 0; --k) {
            if (p >= 0) o[p--] = '/';
            p = obj_uint(o, p, a);
        }
        while (p >= 0) o[p--] = ' ';
    }
    dst[1 + 3 * w] = '\n';
}

}  // namespace o2345
