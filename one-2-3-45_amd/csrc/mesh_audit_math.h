// Per-triangle arithmetic of the mesh audit (mesh_audit.hip), shared with the host check build (tests/hostcheck/mesh_audit_check.hip): normal, area,
// volume term, squared edge lengths, quality, the histogram bin and the crease test.  Everything is fp64, one operation at a time, in the order written
// (the library is built with -ffp-contract=off); a dot product is (x x + y y) + z z.  The host twin (mesh_io.audit_triangles / mesh_audit) spells the same
// operations in numpy and is the definition.
#pragma once
#include "common.h"
#include <math.h>

namespace o2345 {

constexpr double AU_QUALITY_SCALE = 6.928203230275509;      // 4 sqrt(3): an equilateral triangle has quality 1
constexpr int AU_BINS = 10;

struct AuTriangle {
    double n[3], nn;                      // (P1 - P0) x (P2 - P0) and n . n; nn == 0: no area
    double area, vol;                     // 0.5 sqrt(nn); P0 . (P1 x P2)
    double l[3], s;                       // squared lengths of P0P1, P1P2, P2P0; (l01 + l12) + l20
    double q;                             // (4 sqrt(3) area) / s; 0 when s == 0
};

O2345_HD double au_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

O2345_HD void au_sub(const double (&a)[3], const double (&b)[3], double (&r)[3]) { r[0] = a[0] - b[0]; r[1] = a[1] - b[1]; r[2] = a[2] - b[2]; }

O2345_HD void au_cross(const double (&a)[3], const double (&b)[3], double (&r)[3]) {
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}

// n and nn alone: what the crease test needs of the triangle across an edge
O2345_HD double au_normal(const double (&P0)[3], const double (&P1)[3], const double (&P2)[3], double (&n)[3]) {
    double e1[3], e2[3];
    au_sub(P1, P0, e1); au_sub(P2, P0, e2);
    au_cross(e1, e2, n);
    return au_dot(n, n);
}

O2345_HD void au_triangle(const double (&P0)[3], const double (&P1)[3], const double (&P2)[3], AuTriangle& T) {
    double e[3], c[3];
    T.nn = au_normal(P0, P1, P2, T.n);
    T.area = 0.5 * sqrt(T.nn);
    au_cross(P1, P2, c);
    T.vol = au_dot(P0, c);
    au_sub(P1, P0, e); T.l[0] = au_dot(e, e);
    au_sub(P2, P1, e); T.l[1] = au_dot(e, e);
    au_sub(P0, P2, e); T.l[2] = au_dot(e, e);
    T.s = (T.l[0] + T.l[1]) + T.l[2];
    T.q = T.s == 0.0 ? 0.0 : (AU_QUALITY_SCALE * T.area) / T.s;
}

// bin of a quality: min(9, floor(q 10)); -1 for a q that is not >= 0 (it enters no bin and no minimum)
O2345_HD int au_bin(double q) {
    if (!(q >= 0.0)) return -1;
    const double f = floor(q * 10.0);
    return f >= (double)(AU_BINS - 1) ? AU_BINS - 1 : (int)f;
}

// the two triangles of a manifold, consistent edge: creased iff both have an area and their normals are more than a right angle apart
O2345_HD bool au_creased(const double (&n)[3], double nn, const double (&m)[3], double mm) { return nn > 0.0 && mm > 0.0 && au_dot(n, m) < 0.0; }

}  // namespace o2345
