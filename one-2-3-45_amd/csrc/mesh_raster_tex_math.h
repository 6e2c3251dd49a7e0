// Per-pixel arithmetic of the textured shading stage (mesh_raster.hip: k_rs_shade_tex), shared with the host check build
// (tests/hostcheck/mesh_raster_tex_check.hip): the pixel's uv, the four taps and weights of the bilinear fetch, the albedo, the shading normal through the
// file's tangent frame and the headlight term.  Everything is fp64, one operation at a time, in the order written (the library is built with
// -ffp-contract=off); a dot product is (x x + y y) + z z; every result is rounded to float32 once.  The host twin (one-2-3-45_amd/raster.py:
// shade_textured, fetch_texture) spells the same operations in numpy and is the definition; include/o2345.h has the text.  The tangent-frame pieces (dot,
// cross, the usable length, the degenerate mark) are mesh_normalmap_math.h's.
#pragma once
#include "mesh_normalmap_math.h"
#include "mesh_raster_math.h"

namespace o2345 {

constexpr int RT_MAX_SIDE = 16384;                    // of the atlas: a texel index stays below 2^28

struct RtTaps {
    int x[4], y[4];                                   // taps (0,0), (1,0), (0,1), (1,1), clamped to the image
    double w[4];
};

// u = (b0 u0 + b1 u1) + b2 u2, v likewise, of the triangle's six float32 texture coordinates (stored corner order); false: u or v is not finite
O2345_HD bool rt_uv(const double (&b)[3], const float* __restrict__ uv, double& u, double& v) {
    u = (b[0] * (double)uv[0] + b[1] * (double)uv[2]) + b[2] * (double)uv[4];
    v = (b[0] * (double)uv[1] + b[1] * (double)uv[3]) + b[2] * (double)uv[5];
    return rs_finite(u) && rs_finite(v);
}

// clamp(s, 0, hi) in floating point, THEN the conversion: a finite s of any size gives an index inside the image
O2345_HD int rt_index(double s, int hi) {
    const double h = (double)hi;
    return (int)(s < 0.0 ? 0.0 : (s > h ? h : s));
}

// finite u, v -> the four taps and weights of mesh_io.sample_texture on an image of Wt x Ht texels
O2345_HD void rt_taps(double u, double v, int Ht, int Wt, RtTaps& t) {
    const double x = u * (double)Wt - 0.5, y = v * (double)Ht - 0.5;
    const double x0 = floor(x), y0 = floor(y);
    const double fx = x - x0, fy = y - y0;
    t.x[0] = t.x[2] = rt_index(x0 + 0.0, Wt - 1);
    t.x[1] = t.x[3] = rt_index(x0 + 1.0, Wt - 1);
    t.y[0] = t.y[1] = rt_index(y0 + 0.0, Ht - 1);
    t.y[2] = t.y[3] = rt_index(y0 + 1.0, Ht - 1);
    t.w[0] = (1.0 - fx) * (1.0 - fy);
    t.w[1] = fx * (1.0 - fy);
    t.w[2] = (1.0 - fx) * fy;
    t.w[3] = fx * fy;
}

// ((w00 c00 + w10 c10) + w01 c01) + w11 c11 of channels 0 - 2; image: RGBA8 [Ht,Wt], 4-byte aligned, one 4-byte load per tap
O2345_HD void rt_fetch(const uint8_t* __restrict__ image, int Wt, const RtTaps& t, double (&value)[3]) {
    const uint32_t* __restrict__ texel = (const uint32_t*)image;
    uint32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = texel[(long long)t.y[k] * Wt + t.x[k]];
#pragma unroll
    for (int d = 0; d < 3; ++d)
        value[d] = ((t.w[0] * (double)((c[0] >> (8 * d)) & 255u) + t.w[1] * (double)((c[1] >> (8 * d)) & 255u)) + t.w[2] * (double)((c[2] >> (8 * d)) & 255u)) +
                   t.w[3] * (double)((c[3] >> (8 * d)) & 255u);
}

O2345_HD float rt_albedo(double value) { return (float)(value / 255.0); }

// s = the fetched normal texel (channels 0 - 2, 0 .. 255), N float32 [3] and T float32 [4] of the triangle's first corner -> nrm = float32(m / |m|) with
// (x, y, z) = s / 255 * 2 - 1, B = w (N x T), m = (x T + y B) + z N.  False, with nrm = N: the frame carries the degenerate mark, or |m| is zero or not finite
O2345_HD bool rt_normal(const double (&s)[3], const float* __restrict__ N, const float* __restrict__ T, float (&nrm)[3]) {
    const double x = s[0] / 255.0 * 2.0 - 1.0, y = s[1] / 255.0 * 2.0 - 1.0, z = s[2] / 255.0 * 2.0 - 1.0;
    const double Nd[3] = {(double)N[0], (double)N[1], (double)N[2]}, Td[3] = {(double)T[0], (double)T[1], (double)T[2]}, w = (double)T[3];
    double B[3], m[3];
    nm_cross(Nd, Td, B);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        B[d] = w * B[d];
        m[d] = (x * Td[d] + y * B[d]) + z * Nd[d];
    }
    const double l = sqrt(nm_dot(m, m));
    const bool ok = !nm_degenerate_frame(T) && nm_length_ok(l);
#pragma unroll
    for (int d = 0; d < 3; ++d) nrm[d] = ok ? (float)(m[d] / l) : N[d];
    return ok;
}

// The headlight: d = the unit direction of the ray through pixel (px, py) in the mesh's frame, n = nrm / |nrm| (0 for a length that is zero or not
// finite), c = n . d, s = max(0, -c) -> the factor ambient + (1 - ambient) s; back: c > 0
O2345_HD double rt_shade(const RsCamera& cam, int px, int py, const float (&nrm)[3], double ambient, bool& back) {
    const double vx = ((double)px - cam.cx) / cam.fx, vy = ((double)py - cam.cy) / cam.fy;
    double d[3], n[3] = {(double)nrm[0], (double)nrm[1], (double)nrm[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = (cam.R[3 * k] * vx + cam.R[3 * k + 1] * vy) + cam.R[3 * k + 2];
    const double ld = sqrt(nm_dot(d, d)), ln = sqrt(nm_dot(n, n));
    const bool ok = nm_length_ok(ln);
#pragma unroll
    for (int k = 0; k < 3; ++k) { d[k] = d[k] / ld; n[k] = ok ? n[k] / ln : 0.0; }
    const double c = nm_dot(n, d);
    back = c > 0.0;
    return ambient + (1.0 - ambient) * (-c > 0.0 ? -c : 0.0);
}

O2345_HD float rt_lit(float albedo, double factor) { return (float)((double)albedo * factor); }

}  // namespace o2345
