// TEST-ONLY host build of one-2-3-45_amd/csrc/mesh_align_math.h (__host__ __device__): the transform of a point, the closest point on a triangle and
// the point-to-plane terms that the alignment kernel executes, looped on the CPU.  Never loaded by the product package.
#include "../../one-2-3-45_amd/csrc/mesh_align_math.h"

using namespace o2345;
namespace o2345 { void set_error(const char*, ...) {} }

static void corners(const double* verts, const long long* faces, long long t, double (&A)[3], double (&B)[3], double (&C)[3]) {
    for (int d = 0; d < 3; ++d) { A[d] = verts[3 * faces[3 * t] + d]; B[d] = verts[3 * faces[3 * t + 1] + d]; C[d] = verts[3 * faces[3 * t + 2] + d]; }
}

extern "C" {

// moved [n,3] = ma_apply(T [12], points [n,3])
void mac_apply(const double* T, const double* points, long long n, double* moved) {
    double t[12];
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    for (long long i = 0; i < n; ++i) {
        const double p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        double x[3];
        ma_apply(t, p, x);
        for (int d = 0; d < 3; ++d) moved[3 * i + d] = x[d];
    }
}

// every point against its given triangle: d2, region, q [n,3] of md_closest_point, and d2 of md_point_triangle next to it
void mac_closest_point(const double* points, long long n, const double* verts, const long long* faces, const int* triangle, double* d2, double* d2_plain,
                       unsigned char* region, double* q) {
    for (long long i = 0; i < n; ++i) {
        const double p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        double A[3], B[3], C[3], x[3];
        corners(verts, faces, triangle[i], A, B, C);
        int r, r2;
        d2[i] = md_closest_point(p, A, B, C, r, x);
        d2_plain[i] = md_point_triangle(p, A, B, C, r2);
        region[i] = (unsigned char)(r == r2 ? r : 255);
        for (int d = 0; d < 3; ++d) q[3 * i + d] = x[d];
    }
}

// the 35 terms [n,35] of every point x [n,3] with closest point q [n,3] on its given triangle, pivot c [3], weights w [n]
void mac_terms(const double* x, const double* q, long long n, const double* verts, const long long* faces, const int* triangle, const double* c,
               const double* w, double* terms) {
    const double pivot[3] = {c[0], c[1], c[2]};
    for (long long i = 0; i < n; ++i) {
        const double xi[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]}, qi[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
        double A[3], B[3], C[3], J[7], b, term[MA_TERMS];
        corners(verts, faces, triangle[i], A, B, C);
        ma_jacobian(xi, qi, A, B, C, pivot, J, b);
        ma_terms(J, b, w[i], term);
        for (int k = 0; k < MA_TERMS; ++k) terms[MA_TERMS * i + k] = term[k];
    }
}

}  // extern "C"
