// TEST-ONLY host build of one-2-3-45_amd/csrc/mesh_raycast_math.h (__host__ __device__): the segment-triangle hit with its parameter, the rule of the
// nearest hit, the face normal, the frame of a direction and the ends of an occlusion ray that the ray cast kernels execute, looped on the CPU.  A
// stand-alone program: it reads a mesh, segments, directions and a table from a file and writes its results to another, both raw little-endian arrays
// (tests/test_mesh_raycast_hostcheck.py has the layout).  Never loaded by the product package.
#include "../../one-2-3-45_amd/csrc/mesh_raycast_math.h"
#include <stdio.h>
#include <vector>

using namespace o2345;
namespace o2345 { void set_error(const char*, ...) {} }

template <typename T>
static bool read_all(FILE* f, std::vector<T>& a, long long n) { a.resize((size_t)n); return n == 0 || fread(a.data(), sizeof(T), (size_t)n, f) == (size_t)n; }

template <typename T>
static bool write_all(FILE* f, const std::vector<T>& a) { return a.empty() || fwrite(a.data(), sizeof(T), a.size(), f) == a.size(); }

static void row(const std::vector<double>& a, long long i, double (&r)[3]) { r[0] = a[3 * i]; r[1] = a[3 * i + 1]; r[2] = a[3 * i + 2]; }

// in:  int64 nv, nt, ns, nd, S; fp64 max_distance, bias; fp64 verts [nv,3]; int64 faces [nt,3] (in range); fp64 P [ns,3], Q [ns,3]; fp64 dirs [nd,3];
//      fp64 points [nd,3]; fp64 table [S,3]
// out: fp64 t [ns,nt]; int64 hit [ns,nt]; fp64 best [ns]; int64 best_tri [ns] (over the triangles with finite corners and n . n != 0, segments with a
//      non-finite coordinate cast nothing); fp64 normal [nt,3]; fp64 frame [nd,9] = T, B, N; int64 ok [nd]; fp64 rays [nd,S,6] = P, Q_i (frames that
//      are not ok: zeros)
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    long long head[5];
    double scal[2];
    if (fread(head, sizeof(long long), 5, in) != 5 || fread(scal, sizeof(double), 2, in) != 2) return 4;
    const long long nv = head[0], nt = head[1], ns = head[2], nd = head[3], S = head[4];
    std::vector<double> verts, P, Q, dirs, points, table;
    std::vector<long long> faces;
    if (!read_all(in, verts, 3 * nv) || !read_all(in, faces, 3 * nt) || !read_all(in, P, 3 * ns) || !read_all(in, Q, 3 * ns) || !read_all(in, dirs, 3 * nd) ||
        !read_all(in, points, 3 * nd) || !read_all(in, table, 3 * S))
        return 4;
    fclose(in);
    std::vector<double> t((size_t)(ns * nt)), best((size_t)ns), normal((size_t)(3 * nt)), frame((size_t)(9 * nd)), rays((size_t)(6 * nd * S), 0.0);
    std::vector<long long> hit((size_t)(ns * nt)), best_tri((size_t)ns), ok((size_t)nd);
    for (long long k = 0; k < nt; ++k) {
        double A[3], B[3], C[3], n[3];
        row(verts, faces[3 * k], A); row(verts, faces[3 * k + 1], B); row(verts, faces[3 * k + 2], C);
        rc_face_normal(A, B, C, n);
        for (int d = 0; d < 3; ++d) normal[3 * k + d] = n[d];
    }
    for (long long s = 0; s < ns; ++s) {
        double p[3], q[3], b = INFINITY;
        int bt = -1;
        row(P, s, p); row(Q, s, q);
        for (long long k = 0; k < nt; ++k) {
            double A[3], B[3], C[3], tp;
            row(verts, faces[3 * k], A); row(verts, faces[3 * k + 1], B); row(verts, faces[3 * k + 2], C);
            const bool h = rc_segment_triangle(p, q, A, B, C, tp);
            t[s * nt + k] = tp;
            hit[s * nt + k] = h ? 1 : 0;
            bool usable = md_normal2(A, B, C) != 0.0;
            for (int d = 0; d < 3; ++d) usable = usable && fabs(A[d]) <= DBL_MAX && fabs(B[d]) <= DBL_MAX && fabs(C[d]) <= DBL_MAX;
            if (h && usable && rc_segment_finite(p, q)) rc_nearest(tp, (int)k, b, bt);
        }
        best[s] = b;
        best_tri[s] = bt;
    }
    for (long long i = 0; i < nd; ++i) {
        double n[3], p[3], T[3] = {0, 0, 0}, B[3] = {0, 0, 0}, N[3] = {0, 0, 0};
        row(dirs, i, n); row(points, i, p);
        ok[i] = rc_frame(n, T, B, N) ? 1 : 0;
        for (int d = 0; d < 3; ++d) { frame[9 * i + d] = T[d]; frame[9 * i + 3 + d] = B[d]; frame[9 * i + 6 + d] = N[d]; }
        if (!ok[i]) continue;
        for (long long j = 0; j < S; ++j) {
            double a[3], b[3];
            rc_occlusion_ray(p, T, B, N, table[3 * j], table[3 * j + 1], table[3 * j + 2], scal[0], scal[1], a, b);
            for (int d = 0; d < 3; ++d) { rays[6 * (i * S + j) + d] = a[d]; rays[6 * (i * S + j) + 3 + d] = b[d]; }
        }
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 5;
    const bool done = write_all(out, t) && write_all(out, hit) && write_all(out, best) && write_all(out, best_tri) && write_all(out, normal) &&
                      write_all(out, frame) && write_all(out, ok) && write_all(out, rays);
    return fclose(out) == 0 && done ? 0 : 6;
}
