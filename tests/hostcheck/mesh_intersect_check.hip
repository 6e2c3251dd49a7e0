// TEST-ONLY host build of one-2-3-45_amd/csrc/mesh_intersect_math.h (__host__ __device__): the orientation determinant, the segment-triangle crossing, the
// box overlap, the shared indices and the pair test that the self-intersection kernels execute, looped on the CPU.  A stand-alone program: it reads a
// mesh and a list of face pairs from a file and writes its results to another, both raw little-endian arrays (tests/test_mesh_intersect_hostcheck.py
// has the layout).  Never loaded by the product package.
#include "../../one-2-3-45_amd/csrc/mesh_intersect_math.h"
#include <vector>

using namespace o2345;
namespace o2345 { void set_error(const char*, ...) {} }

static void face(const double* verts, const long long* faces, long long t, int (&idx)[3], double (&P)[3][3]) {
    for (int k = 0; k < 3; ++k) {
        idx[k] = (int)faces[3 * t + k];
        for (int d = 0; d < 3; ++d) P[k][d] = verts[3 * faces[3 * t + k] + d];
    }
}

template <typename T>
static bool read_all(FILE* f, std::vector<T>& a, long long n) { a.resize((size_t)n); return n == 0 || fread(a.data(), sizeof(T), (size_t)n, f) == (size_t)n; }

// in:  int64 nv, nt, np; fp64 verts [nv,3]; int64 faces [nt,3]; int64 pairs [np,2] = (t, u)
// out: fp64 orient [np,6] = orient(T0,T1,T2,U_k), k = 0 .. 2, then orient(U0,U1,U2,T_k); int64 flags [np,9] = edge i of t crosses u (i = 0 .. 2, whatever
//      the indices), edge i of u crosses t, boxes overlap, shared indices, the pair test
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    long long head[3];
    if (fread(head, sizeof(long long), 3, in) != 3) return 4;
    const long long nv = head[0], nt = head[1], np = head[2];
    std::vector<double> verts;
    std::vector<long long> faces, pairs;
    if (!read_all(in, verts, 3 * nv) || !read_all(in, faces, 3 * nt) || !read_all(in, pairs, 2 * np)) return 4;
    fclose(in);
    std::vector<double> val((size_t)(6 * np));
    std::vector<long long> flags((size_t)(9 * np));
    for (long long k = 0; k < np; ++k) {
        int it[3], iu[3];
        double T[3][3], U[3][3];
        face(verts.data(), faces.data(), pairs[2 * k], it, T);
        face(verts.data(), faces.data(), pairs[2 * k + 1], iu, U);
        double* o = val.data() + 6 * k;
        long long* g = flags.data() + 9 * k;
        for (int i = 0; i < 3; ++i) {
            o[i] = mi_orient(T[0], T[1], T[2], U[i]);
            o[3 + i] = mi_orient(U[0], U[1], U[2], T[i]);
            g[i] = mi_segment_crosses(T[i], T[(i + 1) % 3], U[0], U[1], U[2]) ? 1 : 0;
            g[3 + i] = mi_segment_crosses(U[i], U[(i + 1) % 3], T[0], T[1], T[2]) ? 1 : 0;
        }
        double lo_t[3], hi_t[3], lo_u[3], hi_u[3];
        for (int d = 0; d < 3; ++d) {
            lo_t[d] = fmin(T[0][d], fmin(T[1][d], T[2][d])); hi_t[d] = fmax(T[0][d], fmax(T[1][d], T[2][d]));
            lo_u[d] = fmin(U[0][d], fmin(U[1][d], U[2][d])); hi_u[d] = fmax(U[0][d], fmax(U[1][d], U[2][d]));
        }
        g[6] = mi_boxes_overlap(lo_t, hi_t, lo_u, hi_u) ? 1 : 0;
        g[7] = mi_shared(it, iu);
        g[8] = mi_pair_intersects(it, T, iu, U) ? 1 : 0;
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 5;
    const bool ok = (val.empty() || fwrite(val.data(), sizeof(double), val.size(), out) == val.size()) &&
                    (flags.empty() || fwrite(flags.data(), sizeof(long long), flags.size(), out) == flags.size());
    return fclose(out) == 0 && ok ? 0 : 6;
}
