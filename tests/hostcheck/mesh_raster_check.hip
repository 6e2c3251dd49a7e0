// TEST-ONLY host build of one-2-3-45_amd/csrc/mesh_raster_math.h (__host__ __device__): the projection, the snap, the skip classes, the edge functions with
// their tie rule and the depth / barycentric step that the rasterizer's kernels execute, looped on the CPU.  A stand-alone program: it reads a camera, a mesh
// and a list of (face, pixel) queries from a file and writes its results to another, both raw little-endian arrays (tests/test_mesh_raster_hostcheck.py has
// the layout).  Never loaded by the product package.
#include "../../one-2-3-45_amd/csrc/mesh_raster_math.h"
#include <vector>

using namespace o2345;
namespace o2345 { void set_error(const char*, ...) {} }

template <typename T>
static bool read_all(FILE* f, std::vector<T>& a, long long n) { a.resize((size_t)n); return n == 0 || fread(a.data(), sizeof(T), (size_t)n, f) == (size_t)n; }
template <typename T>
static bool write_all(FILE* f, const std::vector<T>& a) { return a.empty() || fwrite(a.data(), sizeof(T), a.size(), f) == a.size(); }

// in:  int64 nv, nt, H, W, cull, nq; fp64 camera [17] = R [9] row-major, t [3], fx, fy, cx, cy, near; fp64 verts [nv,3]; int64 faces [nt,3];
//      int64 queries [nq,3] = (face, px, py)
// out: int64 per face [nt,14] = class, sx [3], sy [3], corner [3], px0, py0, px1, py1; fp64 z [nt,3]; int64 per query [nq,4] = w [3], covered; fp64 per
//      query [nq,4] = z, b [3] in computation order -- a query of a face that does not take part or outside the face's box gives zeros
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    long long head[6];
    if (fread(head, sizeof(long long), 6, in) != 6) return 4;
    const long long nv = head[0], nt = head[1], nq = head[5];
    std::vector<double> camera, verts;
    std::vector<long long> faces, queries;
    if (!read_all(in, camera, 17) || !read_all(in, verts, 3 * nv) || !read_all(in, faces, 3 * nt) || !read_all(in, queries, 3 * nq)) return 4;
    fclose(in);
    RsCamera cam{};
    for (int k = 0; k < 9; ++k) cam.R[k] = camera[k];
    for (int k = 0; k < 3; ++k) cam.t[k] = camera[9 + k];
    cam.fx = camera[12]; cam.fy = camera[13]; cam.cx = camera[14]; cam.cy = camera[15]; cam.near = camera[16];
    cam.H = (int)head[2]; cam.W = (int)head[3]; cam.cull = (int)head[4];
    std::vector<RsFace> setup((size_t)nt);
    std::vector<long long> fi((size_t)(14 * nt)), qi((size_t)(4 * nq));
    std::vector<double> fz((size_t)(3 * nt)), qz((size_t)(4 * nq));
    for (long long t = 0; t < nt; ++t) {
        bool in_range = true;
        int idx[3];
        for (int k = 0; k < 3; ++k) {
            const long long i = faces[3 * t + k];
            in_range = in_range && i >= 0 && i < nv;
            idx[k] = (int)i;
        }
        RsFace& f = setup[t];
        long long* o = fi.data() + 14 * t;
        o[0] = rs_setup(cam, verts.data(), in_range, idx, f);
        for (int k = 0; k < 3; ++k) { o[1 + k] = f.sx[k]; o[4 + k] = f.sy[k]; o[7 + k] = f.corner[k]; fz[3 * t + k] = f.z[k]; }
        o[10] = f.px0; o[11] = f.py0; o[12] = f.px1; o[13] = f.py1;
    }
    for (long long q = 0; q < nq; ++q) {
        const long long t = queries[3 * q], px = queries[3 * q + 1], py = queries[3 * q + 2];
        if (t < 0 || t >= nt) return 7;
        const RsFace& f = setup[t];
        if (f.cls != RS_OK || px < f.px0 || px > f.px1 || py < f.py0 || py > f.py1) continue;
        long long w[3];
        double z, b[3];
        const bool inside = rs_edges(f, (int)px, (int)py, w);
        const bool finite = rs_depth(f, w, z, b);
        for (int k = 0; k < 3; ++k) { qi[4 * q + k] = w[k]; qz[4 * q + 1 + k] = b[k]; }
        qi[4 * q + 3] = inside && finite ? 1 : 0;
        qz[4 * q] = z;
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 5;
    const bool ok = write_all(out, fi) && write_all(out, fz) && write_all(out, qi) && write_all(out, qz);
    return fclose(out) == 0 && ok ? 0 : 6;
}
