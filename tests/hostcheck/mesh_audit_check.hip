// TEST-ONLY host build of one-2-3-45_amd/csrc/mesh_audit_math.h (__host__ __device__): the per-triangle arithmetic, the histogram bin and the crease test
// that the audit kernels execute, looped on the CPU.  A stand-alone program: it reads a mesh and a list of triangle pairs from a file and writes its
// results to another, both raw little-endian arrays (tests/test_mesh_audit_hostcheck.py has the layout).  Never loaded by the product package.
#include "../../one-2-3-45_amd/csrc/mesh_audit_math.h"
#include <vector>

using namespace o2345;
namespace o2345 { void set_error(const char*, ...) {} }

static void corners(const double* verts, const long long* faces, long long t, double (&A)[3], double (&B)[3], double (&C)[3]) {
    for (int d = 0; d < 3; ++d) { A[d] = verts[3 * faces[3 * t] + d]; B[d] = verts[3 * faces[3 * t + 1] + d]; C[d] = verts[3 * faces[3 * t + 2] + d]; }
}

template <typename T>
static bool read_all(FILE* f, std::vector<T>& a, long long n) { a.resize((size_t)n); return n == 0 || fread(a.data(), sizeof(T), (size_t)n, f) == (size_t)n; }

// in:  int64 nv, nt, np; fp64 verts [nv,3]; int64 faces [nt,3]; int64 pairs [np,2]
// out: fp64 [nt,11] = n (3), nn, area, vol, l (3), s, q; int64 bin [nt]; int64 creased [np]
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
    std::vector<double> val((size_t)(11 * nt));
    std::vector<long long> bin((size_t)nt), creased((size_t)np);
    for (long long t = 0; t < nt; ++t) {
        double A[3], B[3], C[3];
        corners(verts.data(), faces.data(), t, A, B, C);
        AuTriangle T;
        au_triangle(A, B, C, T);
        double* o = val.data() + 11 * t;
        for (int d = 0; d < 3; ++d) { o[d] = T.n[d]; o[6 + d] = T.l[d]; }
        o[3] = T.nn; o[4] = T.area; o[5] = T.vol; o[9] = T.s; o[10] = T.q;
        bin[(size_t)t] = au_bin(T.q);
    }
    for (long long k = 0; k < np; ++k) {
        double A[3], B[3], C[3], n[3], m[3];
        corners(verts.data(), faces.data(), pairs[2 * k], A, B, C);
        const double nn = au_normal(A, B, C, n);
        corners(verts.data(), faces.data(), pairs[2 * k + 1], A, B, C);
        const double mm = au_normal(A, B, C, m);
        creased[(size_t)k] = au_creased(n, nn, m, mm) ? 1 : 0;
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 5;
    const bool ok = (val.empty() || fwrite(val.data(), sizeof(double), val.size(), out) == val.size()) &&
                    (bin.empty() || fwrite(bin.data(), sizeof(long long), bin.size(), out) == bin.size()) &&
                    (creased.empty() || fwrite(creased.data(), sizeof(long long), creased.size(), out) == creased.size());
    return fclose(out) == 0 && ok ? 0 : 6;
}
