// Per-sample arithmetic of the mesh alignment (mesh_align.hip), shared with the host check build (tests/hostcheck/mesh_align_check.hip): the similarity
// transform of a point and the point-to-plane terms of one matched sample.  Everything is fp64, one operation at a time, in the order written (the library
// is built with -ffp-contract=off); a dot product is (x x + y y) + z z.  The host twin (mesh_io.align_apply / align_sample_terms) spells the same
// operations in numpy and is the definition.
#pragma once
#include "mesh_distance_math.h"

namespace o2345 {

constexpr int MA_MAX_TRANSFORMS = 64;     // transforms of one step
constexpr int MA_COLS = 48;               // doubles of a moments row
constexpr int MA_SUMS = 46;               // of which sums; the last two are 0
constexpr int MA_TERMS = 35;              // w J_i J_j (i <= j, row-major: 28) and w J_i b (7)

// x = M p + t, T the rows of [M | t]: x_k = ((M_k0 p_0 + M_k1 p_1) + M_k2 p_2) + t_k
O2345_HD void ma_apply(const double (&T)[12], const double (&p)[3], double (&x)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = ((T[4 * k] * p[0] + T[4 * k + 1] * p[1]) + T[4 * k + 2] * p[2]) + T[4 * k + 3];
}

// The linearised point-to-plane residual of a moved point x whose closest point on triangle (A, B, C) is q, under a further small similarity about the
// pivot c: x -> c + exp(sigma) R(omega) (x - c) + tau.  With x' = x - c and the unit normal n = ((B - A) x (C - A)) / sqrt(n . n) it is J . u - b for
// u = (omega, tau, sigma): J = (x' x n, n, n . x'), b = n . (q - x).  The sign of n cancels in every product J_i J_j and J_i b.
O2345_HD void ma_jacobian(const double (&x)[3], const double (&q)[3], const double (&A)[3], const double (&B)[3], const double (&C)[3], const double (&c)[3],
                          double (&J)[7], double& b) {
    double e1[3], e2[3], m[3], n[3], xp[3], d[3];
    md_sub(B, A, e1); md_sub(C, A, e2);
    m[0] = e1[1] * e2[2] - e1[2] * e2[1];
    m[1] = e1[2] * e2[0] - e1[0] * e2[2];
    m[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double l = sqrt(md_dot(m, m));
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = m[k] / l;
    md_sub(x, c, xp);
    J[0] = xp[1] * n[2] - xp[2] * n[1];
    J[1] = xp[2] * n[0] - xp[0] * n[2];
    J[2] = xp[0] * n[1] - xp[1] * n[0];
    J[3] = n[0]; J[4] = n[1]; J[5] = n[2];
    J[6] = md_dot(n, xp);
    md_sub(q, x, d);
    b = md_dot(n, d);
}

// the 35 terms of one sample of weight w: (w J_i) J_j for i <= j, row-major, then (w J_i) b
O2345_HD void ma_terms(const double (&J)[7], double b, double w, double (&term)[MA_TERMS]) {
    int at = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const double wj = w * J[i];
#pragma unroll
        for (int j = i; j < 7; ++j) term[at++] = wj * J[j];
        term[28 + i] = wj * b;
    }
}

}  // namespace o2345
