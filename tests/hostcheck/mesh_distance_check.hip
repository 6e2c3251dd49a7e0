// TEST-ONLY host build of one-2-3-45_amd/csrc/mesh_distance_math.h (__host__ __device__): the sample rule and the point - triangle distance that the
// mesh distance kernels execute, looped on the CPU in the kernels' own order.  Never loaded by the product package.
#include "../../one-2-3-45_amd/csrc/mesh_distance_math.h"

using namespace o2345;
namespace o2345 { void set_error(const char*, ...) {} }

static void corners(const double* verts, const long long* faces, long long t, double (&A)[3], double (&B)[3], double (&C)[3]) {
    for (int d = 0; d < 3; ++d) { A[d] = verts[3 * faces[3 * t] + d]; B[d] = verts[3 * faces[3 * t + 1] + d]; C[d] = verts[3 * faces[3 * t + 2] + d]; }
}

extern "C" {

// k[t] of every triangle; spacing <= 0: one sample per triangle
void mdc_levels(const double* verts, const long long* faces, long long nt, double spacing, int* k) {
    for (long long t = 0; t < nt; ++t) {
        double A[3], B[3], C[3];
        corners(verts, faces, t, A, B, C);
        k[t] = md_level(A, B, C, spacing);
    }
}

// the samples of every triangle at the given levels, triangle-major: points [n,3], weights [n]; returns n
long long mdc_samples(const double* verts, const long long* faces, long long nt, const int* k, double* points, double* weights) {
    long long e = 0;
    for (long long t = 0; t < nt; ++t) {
        double A[3], B[3], C[3], p[3];
        corners(verts, faces, t, A, B, C);
        const double w = md_weight(A, B, C, k[t]);
        for (int s = 0; s < k[t] * k[t]; ++s, ++e) {
            md_sample(A, B, C, k[t], s, p);
            for (int d = 0; d < 3; ++d) points[3 * e + d] = p[d];
            weights[e] = w;
        }
    }
    return e;
}

// every point against every triangle with an area, in index order: d2, nearest (the first minimum) and its region
void mdc_closest(const double* points, long long n, const double* verts, const long long* faces, long long nt, double* d2, int* nearest, unsigned char* region) {
    for (long long i = 0; i < n; ++i) {
        const double p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        double best = INFINITY;
        int best_t = -1, best_r = 0;
        for (long long t = 0; t < nt; ++t) {
            double A[3], B[3], C[3];
            corners(verts, faces, t, A, B, C);
            if (md_normal2(A, B, C) == 0.0) continue;
            int r;
            const double x = md_point_triangle(p, A, B, C, r);
            if (x < best) { best = x; best_t = (int)t; best_r = r; }
        }
        d2[i] = best; nearest[i] = best_t; region[i] = (unsigned char)best_r;
    }
}

int mdc_cell_index(double x, double origin, double cell, int n) { return md_cell_index(x, origin, cell, n); }

}  // extern "C"
