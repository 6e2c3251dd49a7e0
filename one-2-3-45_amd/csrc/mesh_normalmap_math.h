// Arithmetic of the tangent-space normal map (mesh_texture.hip: k_tex_frames, k_tex_normal_pack), shared with the host check build
// (tests/hostcheck/mesh_normalmap_check.hip): the tangent frame of one triangle from the file's own float32 positions and texture coordinates, and one
// RGBA8 texel from a raw SDF gradient and that frame.  Everything is fp64, one operation at a time, in the order written (the library is built with
// -ffp-contract=off); a dot product is (x x + y y) + z z; square roots and divisions are IEEE.  The host twin (mesh_io.texture_frames /
// pack_normal_map) spells the same operations in numpy and is the definition.
#pragma once
#include "common.h"
#include <math.h>

namespace o2345 {

enum { NM_BAD_GRADIENT = 1, NM_BACK_FACING = 2 };         // nm_texel's flags

O2345_HD double nm_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

O2345_HD void nm_cross(const double (&a)[3], const double (&b)[3], double (&r)[3]) {
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}

// a length that a vector can be divided by: neither zero, nor an infinity, nor a NaN
O2345_HD bool nm_length_ok(double l) { return l > 0.0 && l < (double)INFINITY; }

// The frame of one triangle: pos = its three float32 positions (asset frame), uv = its three float32 texture coordinates -> N float32 [3], the unit
// front-face normal of the file's winding, and T float32 [4] = (unit tangent along increasing u, orthogonal to N; w = +1 or -1 such that w (N x T) points
// along DEcreasing v: row 0 of the image is on top and green is up).  False, with N = (0, 1, 0) and T = (1, -0, 0, 1), for a degenerate triangle:
// |e1 x e2|, det or |Pu - N (N . Pu)| zero or not finite.  The NEGATIVE zero of T.y is the mark that the texel pass knows a degenerate triangle by: the
// value is the 0 of the definition, and a sound triangle never carries it, because each of its float32 components has + 0 added, which turns a negative
// zero into a positive one and changes nothing else.  (A flat, axis-aligned triangle has the frame (0, 1, 0), (1, 0, 0, 1) for good reasons.)
O2345_HD bool nm_frame(const float* __restrict__ pos, const float* __restrict__ uv, float (&N)[3], float (&T)[4]) {
    double e1[3], e2[3], c[3], n[3], Pu[3], Pv[3], tv[3], t[3], b[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        e1[d] = (double)pos[3 + d] - (double)pos[d];
        e2[d] = (double)pos[6 + d] - (double)pos[d];
    }
    nm_cross(e1, e2, c);
    const double l = sqrt(nm_dot(c, c));
    const double du1 = (double)uv[2] - (double)uv[0], dv1 = (double)uv[3] - (double)uv[1];
    const double du2 = (double)uv[4] - (double)uv[0], dv2 = (double)uv[5] - (double)uv[1];
    const double det = du1 * dv2 - du2 * dv1;
    bool ok = nm_length_ok(l) && nm_length_ok(fabs(det));
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        n[d] = c[d] / l;
        Pu[d] = (e1[d] * dv2 - e2[d] * dv1) / det;
        Pv[d] = (e2[d] * du1 - e1[d] * du2) / det;
    }
    const double np = nm_dot(n, Pu);
#pragma unroll
    for (int d = 0; d < 3; ++d) tv[d] = Pu[d] - n[d] * np;
    const double lt = sqrt(nm_dot(tv, tv));
    ok = ok && nm_length_ok(lt);
#pragma unroll
    for (int d = 0; d < 3; ++d) { t[d] = tv[d] / lt; Pv[d] = -Pv[d]; }
    nm_cross(n, t, b);
    const double w = nm_dot(b, Pv) >= 0.0 ? 1.0 : -1.0;
    N[0] = ok ? (float)n[0] + 0.f : 0.f; N[1] = ok ? (float)n[1] + 0.f : 1.f; N[2] = ok ? (float)n[2] + 0.f : 0.f;
    T[0] = ok ? (float)t[0] + 0.f : 1.f; T[1] = ok ? (float)t[1] + 0.f : -0.f; T[2] = ok ? (float)t[2] + 0.f : 0.f; T[3] = ok ? (float)w : 1.f;
    return ok;
}

// nm_frame's mark of a degenerate triangle: T.y is a negative zero
O2345_HD bool nm_degenerate_frame(const float* __restrict__ T) { return T[1] == 0.f && __builtin_signbit(T[1]); }

// floor((x 127.5 + 127.5) + 0.5) clamped to [0, 255]; a NaN gives 0
O2345_HD uint8_t nm_channel(double x) {
    const double v = floor((x * 127.5 + 127.5) + 0.5);
    return (uint8_t)(v >= 0.0 ? (v <= 255.0 ? v : 255.0) : 0.0);
}

// One texel: g = the raw SDF gradient float32 [3] at the texel's surface point, R = the 3x3 of trans_mat (row-major float32 [9]) or null, N / T = the
// frame of the owner triangle as the file holds it -> rgba.  n = g through the operations of mesh_normal_f32 (normalise; through R and renormalise; y and
// z exchanged), kept in fp64; B = w (N x T); (x, y, z) = (n . T, n . B, n . N), one nm_channel each, alpha 255.  (128, 128, 255, 255) for a frame marked
// degenerate and for a gradient without a usable length.  Returns NM_BAD_GRADIENT for such a gradient (whatever the frame), NM_BACK_FACING for z < 0.
O2345_HD int nm_texel(const float* __restrict__ g, const float* __restrict__ R, const float* __restrict__ N, const float* __restrict__ T, uint8_t (&rgba)[4]) {
    double v[3] = {(double)g[0], (double)g[1], (double)g[2]};
    double l = sqrt(nm_dot(v, v));
    bool ok = nm_length_ok(l);
    if (ok) {
        v[0] /= l; v[1] /= l; v[2] /= l;
        if (R) {
            double r[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) r[k] = ((double)R[3 * k] * v[0] + (double)R[3 * k + 1] * v[1]) + (double)R[3 * k + 2] * v[2];
            l = sqrt(nm_dot(r, r));
            ok = nm_length_ok(l);
            v[0] = r[0] / l; v[1] = r[1] / l; v[2] = r[2] / l;
        }
    }
    rgba[0] = 128; rgba[1] = 128; rgba[2] = 255; rgba[3] = 255;
    if (!ok) return NM_BAD_GRADIENT;
    if (nm_degenerate_frame(T)) return 0;
    const double n[3] = {v[0], v[2], v[1]};
    const double Nd[3] = {(double)N[0], (double)N[1], (double)N[2]}, Td[3] = {(double)T[0], (double)T[1], (double)T[2]}, w = (double)T[3];
    double B[3];
    nm_cross(Nd, Td, B);
    B[0] = w * B[0]; B[1] = w * B[1]; B[2] = w * B[2];
    const double z = nm_dot(n, Nd);
    rgba[0] = nm_channel(nm_dot(n, Td));
    rgba[1] = nm_channel(nm_dot(n, B));
    rgba[2] = nm_channel(z);
    return z < 0.0 ? NM_BACK_FACING : 0;
}

}  // namespace o2345
