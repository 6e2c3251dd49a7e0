// Per-element arithmetic of the quadric-error simplification (mesh_simplify.hip), shared with the host check build (tests/hostcheck/mesh_simplify_check.hip):
// the quadric of a triangle, the error of a point under a quadric, and the flip test.  Everything is fp64, one operation at a time, in the order written
// (the library is built with -ffp-contract=off); a dot product is (x x + y y) + z z.  The host twin (mesh_io.simplify_quadrics / simplify_error /
// simplify_keeps_side) spells the same operations in numpy and is the definition.
#pragma once
#include "common.h"
#include <math.h>

namespace o2345 {

constexpr int MS_Q = 10;                  // entries of a symmetric 4 x 4: xx xy xz xd yy yz yd zz zd dd

// n = (P1 - P0) x (P2 - P0)
O2345_HD void ms_normal(const double (&P0)[3], const double (&P1)[3], const double (&P2)[3], double (&n)[3]) {
    const double e1[3] = {P1[0] - P0[0], P1[1] - P0[1], P1[2] - P0[2]}, e2[3] = {P2[0] - P0[0], P2[1] - P0[1], P2[2] - P0[2]};
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

// the area-weighted plane quadric of a triangle: with nn = n . n > 0, s = 0.5 / sqrt(nn) and d = -(n . P0), entry = (a b) s over (nx, ny, nz, d);
// a triangle without an area (or with a non-finite normal) contributes zeros
O2345_HD void ms_triangle_quadric(const double (&P0)[3], const double (&P1)[3], const double (&P2)[3], double (&K)[MS_Q]) {
    double n[3];
    ms_normal(P0, P1, P2, n);
    const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (!(nn > 0.0)) {
#pragma unroll
        for (int i = 0; i < MS_Q; ++i) K[i] = 0.0;
        return;
    }
    const double s = 0.5 / sqrt(nn);
    const double c[4] = {n[0], n[1], n[2], -((n[0] * P0[0] + n[1] * P0[1]) + n[2] * P0[2])};
    K[0] = (c[0] * c[0]) * s; K[1] = (c[0] * c[1]) * s; K[2] = (c[0] * c[2]) * s; K[3] = (c[0] * c[3]) * s;
    K[4] = (c[1] * c[1]) * s; K[5] = (c[1] * c[2]) * s; K[6] = (c[1] * c[3]) * s;
    K[7] = (c[2] * c[2]) * s; K[8] = (c[2] * c[3]) * s;
    K[9] = (c[3] * c[3]) * s;
}

// p^T Q p for p = (x, y, z, 1): the ONE expression of the definition; the cost of a collapse is max(0, .) of it
O2345_HD double ms_error(const double (&q)[MS_Q], const double (&p)[3]) {
    const double x = p[0], y = p[1], z = p[2];
    const double r0 = ((q[0] * x + q[1] * y) + q[2] * z) + q[3];
    const double r1 = ((q[1] * x + q[4] * y) + q[5] * z) + q[6];
    const double r2 = ((q[2] * x + q[5] * y) + q[7] * z) + q[8];
    const double r3 = ((q[3] * x + q[6] * y) + q[8] * z) + q[9];
    return ((x * r0 + y * r1) + z * r2) + r3;
}

// the flip test: does triangle (P0, P1, P2) keep its side when corner `corner` moves to Pu?  n . n' > 0; a zero normal on either side fails
O2345_HD bool ms_keeps_side(const double (&P0)[3], const double (&P1)[3], const double (&P2)[3], int corner, const double (&Pu)[3]) {
    double a[3], b[3];
    ms_normal(P0, P1, P2, a);
    if (corner == 0) ms_normal(Pu, P1, P2, b);
    else if (corner == 1) ms_normal(P0, Pu, P2, b);
    else ms_normal(P0, P1, Pu, b);
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2] > 0.0;
}

// the biased exponent field of a non-negative double: the bin of a cost (cost 0 -> bin 0)
O2345_HD int ms_bin(double cost) {
    unsigned long long b;
    __builtin_memcpy(&b, &cost, 8);
    return (int)((b >> 52) & 0x7FF);
}

}  // namespace o2345
