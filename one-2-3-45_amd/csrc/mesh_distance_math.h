// Per-element arithmetic of the mesh-to-mesh distance (mesh_distance.hip), shared with the host check build (tests/hostcheck/mesh_distance_check.hip):
// the subdivision level of a triangle, the surface sample and its weight, and the squared distance from a point to a triangle.  Everything is fp64, one
// operation at a time, in the order written (the library is built with -ffp-contract=off); a dot product is (x x + y y) + z z.  The host twin
// (mesh_io.surface_samples / closest_point_triangle) spells the same operations in numpy and is the definition.
#pragma once
#include "common.h"
#include <math.h>

namespace o2345 {

constexpr int MD_MAX_LEVEL = 64;          // a triangle is split into at most 64^2 sub-triangles

O2345_HD double md_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

O2345_HD void md_sub(const double (&a)[3], const double (&b)[3], double (&r)[3]) { r[0] = a[0] - b[0]; r[1] = a[1] - b[1]; r[2] = a[2] - b[2]; }

// n = (P1 - P0) x (P2 - P0) -> n . n; a triangle with n . n == 0 has no area: weight 0 as a source of samples, no part as a target
O2345_HD double md_normal2(const double (&P0)[3], const double (&P1)[3], const double (&P2)[3]) {
    double e1[3], e2[3], n[3];
    md_sub(P1, P0, e1); md_sub(P2, P0, e2);
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    return md_dot(n, n);
}

// k of a triangle at `spacing` (<= 0: one sample per triangle): the smallest k in [1, 64] with (k spacing)(k spacing) >= L2, L2 the largest squared edge
// length, and 64 if there is none.  No square root and no division.
O2345_HD int md_level(const double (&P0)[3], const double (&P1)[3], const double (&P2)[3], double spacing) {
    if (!(spacing > 0.0)) return 1;
    double e[3];
    md_sub(P1, P0, e); double L2 = md_dot(e, e);
    md_sub(P2, P1, e); double l = md_dot(e, e); if (l > L2) L2 = l;
    md_sub(P0, P2, e); l = md_dot(e, e); if (l > L2) L2 = l;
    int k = 1;
    for (; k < MD_MAX_LEVEL; ++k) {
        const double ks = (double)k * spacing;
        if (ks * ks >= L2) break;
    }
    return k;
}

// sample s in [0, k^2) of a triangle split regularly into k^2 sub-triangles, at their centroids: the k (k + 1) / 2 upright ones first (rows j = 0 .. k - 1
// of i = 0 .. k - 1 - j: w1 = (3 i + 1) / (3 k), w2 = (3 j + 1) / (3 k)), then the inverted ones (rows j = 0 .. k - 2 of i = 0 .. k - 2 - j: w1 = (3 i + 2)
// / (3 k), w2 = (3 j + 2) / (3 k)); w0 = (1 - w1) - w2, p = (w0 P0 + w1 P1) + w2 P2
O2345_HD void md_sample(const double (&P0)[3], const double (&P1)[3], const double (&P2)[3], int k, int s, double (&p)[3]) {
    const int upright = k * (k + 1) / 2;
    int add = 1, row = k;
    if (s >= upright) { s -= upright; add = 2; row = k - 1; }
    int j = 0;
    while (s >= row - j) { s -= row - j; ++j; }
    const double w1 = (double)(3 * s + add) / (double)(3 * k), w2 = (double)(3 * j + add) / (double)(3 * k);
    const double w0 = (1.0 - w1) - w2;
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] = (w0 * P0[d] + w1 * P1[d]) + w2 * P2[d];
}

// weight of every sample of a triangle at level k: area / k^2, area = 0.5 sqrt(n . n)
O2345_HD double md_weight(const double (&P0)[3], const double (&P1)[3], const double (&P2)[3], int k) {
    return 0.5 * sqrt(md_normal2(P0, P1, P2)) / (double)(k * k);
}

// |p - q|^2 and q, the point of triangle (A, B, C) closest to p: the region walk of Ericson, Real-Time Collision Detection 5.1.5, in the book's order;
// region: 0 vertex A, 1 vertex B, 2 edge AB, 3 vertex C, 4 edge AC, 5 edge BC, 6 face.  At a vertex q is that corner and d2 is |p - corner|^2 as computed
// for the region tests: the distance never depends on whether q is wanted
O2345_HD double md_closest_point(const double (&p)[3], const double (&A)[3], const double (&B)[3], const double (&C)[3], int& region, double (&q)[3]) {
    double ab[3], ac[3], ap[3], d[3];
    md_sub(B, A, ab); md_sub(C, A, ac); md_sub(p, A, ap);
    const double d1 = md_dot(ab, ap), d2 = md_dot(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) { region = 0; q[0] = A[0]; q[1] = A[1]; q[2] = A[2]; return md_dot(ap, ap); }
    double bp[3];
    md_sub(p, B, bp);
    const double d3 = md_dot(ab, bp), d4 = md_dot(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) { region = 1; q[0] = B[0]; q[1] = B[1]; q[2] = B[2]; return md_dot(bp, bp); }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = A[k] + v * ab[k];
        region = 2;
        md_sub(p, q, d);
        return md_dot(d, d);
    }
    double cp[3];
    md_sub(p, C, cp);
    const double d5 = md_dot(ab, cp), d6 = md_dot(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) { region = 3; q[0] = C[0]; q[1] = C[1]; q[2] = C[2]; return md_dot(cp, cp); }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double w = d2 / (d2 - d6);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = A[k] + w * ac[k];
        region = 4;
        md_sub(p, q, d);
        return md_dot(d, d);
    }
    const double va = d3 * d6 - d5 * d4;
    const double s43 = d4 - d3, s56 = d5 - d6;
    if (va <= 0.0 && s43 >= 0.0 && s56 >= 0.0) {
        const double w = s43 / (s43 + s56);
        double bc[3];
        md_sub(C, B, bc);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = B[k] + w * bc[k];
        region = 5;
        md_sub(p, q, d);
        return md_dot(d, d);
    }
    const double den = 1.0 / ((va + vb) + vc);
    const double v = vb * den, w = vc * den;
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = (A[k] + ab[k] * v) + ac[k] * w;
    region = 6;
    md_sub(p, q, d);
    return md_dot(d, d);
}

// the distance alone: what the query walks with
O2345_HD double md_point_triangle(const double (&p)[3], const double (&A)[3], const double (&B)[3], const double (&C)[3], int& region) {
    double q[3];
    return md_closest_point(p, A, B, C, region, q);
}

// ---- the uniform grid over a target mesh ---------------------------------------------------------------------------------------------------------
// Cells are the boxes of the lattice of multiples of `cell`: origin o = floor(lo / cell) cell per axis (lo: the mesh's lower bound), n cells per axis.
// The cell index of a coordinate is ONE monotone function, used for registering a triangle's bounding box and for placing a query alike.
struct MdGridHead {
    double origin[3], cell, scale;        // scale: the largest absolute coordinate of the grid's box
    int dims[3], n_cells;
    long long n_entries, cell_start_bytes;          // entries behind the cell_start array of n_cells + 1 ints padded to cell_start_bytes
};

O2345_HD int md_cell_index(double x, double origin, double cell, int n) {
    const double f = floor((x - origin) / cell);
    return f >= (double)(n - 1) ? n - 1 : (f > 0.0 ? (int)f : 0);         // a NaN lands in cell 0
}

}  // namespace o2345
