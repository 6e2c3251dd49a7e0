// Per-ray arithmetic of the ray cast and of the ambient occlusion (mesh_raycast.hip), shared with the host check build
// (tests/hostcheck/mesh_raycast_check.hip): the parameter of a hit, the rule of the nearest hit, the face normal of an owner triangle, the frame of a
// direction, the world direction of a table entry and the two ends of an occlusion ray.  Everything is fp64, one operation at a time, in the order
// written (the library is built with -ffp-contract=off); a dot product is (x x + y y) + z z.  The hit itself is mi_segment_hit (mesh_intersect_math.h).
// The host twin (mesh_io.segment_hits / ray_frame / mesh_occlusion) spells the same operations in numpy and is the definition.
#pragma once
#include "mesh_distance_math.h"
#include "mesh_intersect_math.h"
#include <float.h>

namespace o2345 {

// all six coordinates finite: a segment with another one casts nothing
O2345_HD bool rc_segment_finite(const double (&P)[3], const double (&Q)[3]) {
    return fabs(P[0]) <= DBL_MAX && fabs(P[1]) <= DBL_MAX && fabs(P[2]) <= DBL_MAX && fabs(Q[0]) <= DBL_MAX && fabs(Q[1]) <= DBL_MAX && fabs(Q[2]) <= DBL_MAX;
}

// the segment P -> Q against the triangle (A, B, C) in stored order -> hit, and t = sP / (sP - sQ): in (0, 1) up to rounding, or a NaN where the
// determinants overflow
O2345_HD bool rc_segment_triangle(const double (&P)[3], const double (&Q)[3], const double (&A)[3], const double (&B)[3], const double (&C)[3], double& t) {
    double sP, sQ;
    const bool hit = mi_segment_hit(P, Q, A, B, C, sP, sQ);
    t = sP / (sP - sQ);
    return hit;
}

// the nearest hit so far <- a hit at t of triangle tri: the smaller t, among equal t the smaller index; a NaN never wins.  Independent of the order of
// the visits, and of visiting a triangle twice
O2345_HD void rc_nearest(double t, int tri, double& best, int& best_tri) {
    if (t < best || (t == best && tri < best_tri)) { best = t; best_tri = tri; }
}

// n = (P1 - P0) x (P2 - P0), the corners in stored order
O2345_HD void rc_face_normal(const double (&P0)[3], const double (&P1)[3], const double (&P2)[3], double (&n)[3]) {
    double e1[3], e2[3];
    md_sub(P1, P0, e1); md_sub(P2, P0, e2);
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

// the frame (T, B, N) of a direction n: false when its length is zero or not finite.  The branch-free basis of Duff et al., "Building an orthonormal
// basis, revisited" (JCGT 2017): + - * / and one correctly rounded square root
O2345_HD bool rc_frame(const double (&n)[3], double (&T)[3], double (&B)[3], double (&N)[3]) {
    const double len = sqrt(md_dot(n, n));
    if (!(len > 0.0 && len <= DBL_MAX)) return false;
    N[0] = n[0] / len; N[1] = n[1] / len; N[2] = n[2] / len;
    const double s = copysign(1.0, N[2]);
    const double a = -1.0 / (s + N[2]);
    const double b = (N[0] * N[1]) * a;
    T[0] = 1.0 + (s * N[0]) * (N[0] * a); T[1] = s * b; T[2] = -(s * N[0]);
    B[0] = b; B[1] = s + (N[1] * N[1]) * a; B[2] = -N[1];
    return true;
}

// the ray of table entry (x, y, z) from p: P = p + bias N, d = (x T + y B) + z N, Q = P + max_distance d
O2345_HD void rc_occlusion_ray(const double (&p)[3], const double (&T)[3], const double (&B)[3], const double (&N)[3], double x, double y, double z,
                               double max_distance, double bias, double (&P)[3], double (&Q)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        P[k] = p[k] + bias * N[k];
        const double d = (x * T[k] + y * B[k]) + z * N[k];
        Q[k] = P[k] + max_distance * d;
    }
}

}  // namespace o2345
