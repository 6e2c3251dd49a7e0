// Per-pair arithmetic of the self-intersection report (mesh_intersect.hip), shared with the host check build (tests/hostcheck/mesh_intersect_check.hip):
// the orientation determinant, the segment-triangle crossing, the overlap of two closed boxes, the shared indices of two faces and the pair test.
// Everything is fp64, one operation at a time, in the order written (the library is built with -ffp-contract=off); only comparisons decide.  The host
// twin (mesh_io.intersect_orient / segment_crosses_triangle / triangles_intersect) spells the same operations in numpy and is the definition.
#pragma once
#include "common.h"
#include <math.h>

namespace o2345 {

// a = A - D, b = B - D, c = C - D -> a . (b x c) as (a_x X + a_y Y) + a_z Z: six times the signed volume of the tetrahedron, unfiltered
O2345_HD double mi_orient(const double (&A)[3], const double (&B)[3], const double (&C)[3], const double (&D)[3]) {
    const double ax = A[0] - D[0], ay = A[1] - D[1], az = A[2] - D[2];
    const double bx = B[0] - D[0], by = B[1] - D[1], bz = B[2] - D[2];
    const double cx = C[0] - D[0], cy = C[1] - D[1], cz = C[2] - D[2];
    const double X = by * cz - bz * cy;
    const double Y = bz * cx - bx * cz;
    const double Z = bx * cy - by * cx;
    return (ax * X + ay * Y) + az * Z;
}

// the segment PQ crosses the triangle (A, B, C): P and Q strictly on opposite sides of its plane, and the three determinants around the segment all
// > 0 or all < 0.  A zero or a NaN anywhere: no crossing.  (The last three are skipped when the first two decide: a flag, not a value, is the result.)
// mi_segment_hit also hands out the two plane determinants sP and sQ: the ray cast (mesh_raycast_math.h) takes its parameter from them.
O2345_HD bool mi_segment_hit(const double (&P)[3], const double (&Q)[3], const double (&A)[3], const double (&B)[3], const double (&C)[3], double& sP,
                             double& sQ) {
    sP = mi_orient(A, B, C, P);
    sQ = mi_orient(A, B, C, Q);
    if (!((sP > 0.0 && sQ < 0.0) || (sP < 0.0 && sQ > 0.0))) return false;
    const double o1 = mi_orient(P, Q, A, B), o2 = mi_orient(P, Q, B, C), o3 = mi_orient(P, Q, C, A);
    return (o1 > 0.0 && o2 > 0.0 && o3 > 0.0) || (o1 < 0.0 && o2 < 0.0 && o3 < 0.0);
}

O2345_HD bool mi_segment_crosses(const double (&P)[3], const double (&Q)[3], const double (&A)[3], const double (&B)[3], const double (&C)[3]) {
    double sP, sQ;
    return mi_segment_hit(P, Q, A, B, C, sP, sQ);
}

// closed boxes: lo_t <= hi_u and lo_u <= hi_t on every axis
O2345_HD bool mi_boxes_overlap(const double (&lo_t)[3], const double (&hi_t)[3], const double (&lo_u)[3], const double (&hi_u)[3]) {
    return lo_t[0] <= hi_u[0] && lo_u[0] <= hi_t[0] && lo_t[1] <= hi_u[1] && lo_u[1] <= hi_t[1] && lo_t[2] <= hi_u[2] && lo_u[2] <= hi_t[2];
}

// how many indices of t are indices of u (both faces have three distinct indices)
O2345_HD int mi_shared(const int (&t)[3], const int (&u)[3]) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) n += (t[i] == u[0] || t[i] == u[1] || t[i] == u[2]) ? 1 : 0;
    return n;
}

// some edge (X[i], X[(i + 1) % 3]) of face X, neither end an index of face Y, crosses Y (corners in stored order)
O2345_HD bool mi_edges_cross(const int (&ix)[3], const double (&X)[3][3], const int (&iy)[3], const double (&Y)[3][3]) {
    bool hit = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3;
        const bool free_edge = ix[i] != iy[0] && ix[i] != iy[1] && ix[i] != iy[2] && ix[j] != iy[0] && ix[j] != iy[1] && ix[j] != iy[2];
        if (free_edge && mi_segment_crosses(X[i], X[j], Y[0], Y[1], Y[2])) hit = true;
    }
    return hit;
}

// a candidate pair (at most one shared index) intersects: the edges of t against u, then the edges of u against t
O2345_HD bool mi_pair_intersects(const int (&it)[3], const double (&T)[3][3], const int (&iu)[3], const double (&U)[3][3]) {
    return mi_edges_cross(it, T, iu, U) || mi_edges_cross(iu, U, it, T);
}

}  // namespace o2345
