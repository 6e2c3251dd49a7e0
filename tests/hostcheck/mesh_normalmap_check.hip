// TEST-ONLY host build of one-2-3-45_amd/csrc/mesh_normalmap_math.h (__host__ __device__): the tangent frame of a triangle and the normal-map texel that
// the kernels of mesh_texture.hip execute, looped on the CPU.  A stand-alone program: it reads triangles and texels from a file and writes its results
// to another, both raw little-endian arrays (tests/test_mesh_normal_map_hostcheck.py has the layout).  Never loaded by the product package.
#include "../../one-2-3-45_amd/csrc/mesh_normalmap_math.h"
#include <vector>

using namespace o2345;
namespace o2345 { void set_error(const char*, ...) {} }

template <typename T>
static bool read_all(FILE* f, std::vector<T>& a, long long n) { a.resize((size_t)n); return n == 0 || fread(a.data(), sizeof(T), (size_t)n, f) == (size_t)n; }

template <typename T>
static bool write_all(FILE* f, const std::vector<T>& a) { return a.empty() || fwrite(a.data(), sizeof(T), a.size(), f) == a.size(); }

// in:  int64 nt, ne, has_rotation; float32 positions [3 nt,3], uv [3 nt,2], grad [ne,3], rotation [9]; int64 owner [ne] (the triangle of every texel)
// out: float32 normals [nt,3], tangents [nt,4]; int64 ok [nt]; uint8 rgba [ne,4]; int64 flags [ne]
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    long long head[3];
    if (fread(head, sizeof(long long), 3, in) != 3) return 4;
    const long long nt = head[0], ne = head[1];
    std::vector<float> pos, uv, grad, rot;
    std::vector<long long> owner;
    if (!read_all(in, pos, 9 * nt) || !read_all(in, uv, 6 * nt) || !read_all(in, grad, 3 * ne) || !read_all(in, rot, 9) || !read_all(in, owner, ne)) return 4;
    fclose(in);
    std::vector<float> nrm((size_t)(3 * nt)), tan((size_t)(4 * nt));
    std::vector<long long> ok((size_t)nt), flags((size_t)ne);
    std::vector<uint8_t> rgba((size_t)(4 * ne));
    for (long long t = 0; t < nt; ++t) {
        float N[3], T[4];
        ok[(size_t)t] = nm_frame(pos.data() + 9 * t, uv.data() + 6 * t, N, T) ? 1 : 0;
        for (int d = 0; d < 3; ++d) nrm[(size_t)(3 * t + d)] = N[d];
        for (int d = 0; d < 4; ++d) tan[(size_t)(4 * t + d)] = T[d];
    }
    for (long long e = 0; e < ne; ++e) {
        const long long t = owner[(size_t)e];
        if (t < 0 || t >= nt) return 7;
        uint8_t o[4];
        flags[(size_t)e] = nm_texel(grad.data() + 3 * e, head[2] ? rot.data() : nullptr, nrm.data() + 3 * t, tan.data() + 4 * t, o);
        for (int d = 0; d < 4; ++d) rgba[(size_t)(4 * e + d)] = o[d];
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 5;
    const bool good = write_all(out, nrm) && write_all(out, tan) && write_all(out, ok) && write_all(out, rgba) && write_all(out, flags);
    return fclose(out) == 0 && good ? 0 : 6;
}
