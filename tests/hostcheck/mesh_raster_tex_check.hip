// TEST-ONLY host build of one-2-3-45_amd/csrc/mesh_raster_tex_math.h (__host__ __device__): the pixel's uv, the four taps and weights, the fetch, the albedo,
// the normal through the tangent frame and the headlight that the textured shading kernel executes, looped on the CPU.  A stand-alone program: it reads a
// camera, the images and a list of pixel queries from a file and writes its results to another, both raw little-endian arrays
// (tests/test_mesh_raster_textured_hostcheck.py has the layout).  Never loaded by the product package.
#include "../../one-2-3-45_amd/csrc/mesh_raster_tex_math.h"
#include <vector>

using namespace o2345;
namespace o2345 { void set_error(const char*, ...) {} }

template <typename T>
static bool read_all(FILE* f, std::vector<T>& a, long long n) { a.resize((size_t)n); return n == 0 || fread(a.data(), sizeof(T), (size_t)n, f) == (size_t)n; }
template <typename T>
static bool write_all(FILE* f, const std::vector<T>& a) { return a.empty() || fwrite(a.data(), sizeof(T), a.size(), f) == a.size(); }

// in:  int64 n, Ht, Wt, mapped; fp64 camera [14] = R [9] row-major, fx, fy, cx, cy, ambient; uint8 image [Ht,Wt,4]; uint8 normal image [Ht,Wt,4] when
//      mapped; fp64 per query [n,5] = px, py, bary [3]; float32 per query [n,13] = uv [6], N [3], T [4] (not mapped: N is the pixel's shading normal)
// out: fp64 per query [n,16] = good, u, v, w [4], value [3], s [3], factor, back, ok; int64 [n,8] = tap x [4], y [4]; float32 [n,9] = albedo, nrm, lit --
//      a query whose uv is not finite gives zeros behind u and v
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    long long head[4];
    if (fread(head, sizeof(long long), 4, in) != 4) return 4;
    const long long n = head[0];
    const int Ht = (int)head[1], Wt = (int)head[2];
    const bool mapped = head[3] != 0;
    if (n < 0 || Ht < 1 || Wt < 1 || Ht > RT_MAX_SIDE || Wt > RT_MAX_SIDE) return 4;
    std::vector<double> camera, qd;
    std::vector<uint32_t> image, nimage;                                    // 4-byte aligned, as the entry demands
    std::vector<float> qf;
    if (!read_all(in, camera, 14) || !read_all(in, image, (long long)Ht * Wt) || !read_all(in, nimage, mapped ? (long long)Ht * Wt : 0) ||
        !read_all(in, qd, 5 * n) || !read_all(in, qf, 13 * n))
        return 4;
    fclose(in);
    RsCamera cam{};
    for (int k = 0; k < 9; ++k) cam.R[k] = camera[k];
    cam.fx = camera[9]; cam.fy = camera[10]; cam.cx = camera[11]; cam.cy = camera[12];
    const double ambient = camera[13];
    std::vector<double> od((size_t)(16 * n));
    std::vector<long long> oi((size_t)(8 * n));
    std::vector<float> of((size_t)(9 * n));
    for (long long q = 0; q < n; ++q) {
        const double* d = qd.data() + 5 * q;
        const float* f = qf.data() + 13 * q;
        double* o = od.data() + 16 * q;
        const double b[3] = {d[2], d[3], d[4]};
        double u, v;
        const bool good = rt_uv(b, f, u, v);
        o[0] = good ? 1.0 : 0.0; o[1] = u; o[2] = v;
        if (!good) continue;
        RtTaps t;
        double value[3], s[3] = {0.0, 0.0, 0.0};
        float albedo[3], nrm[3] = {f[6], f[7], f[8]};
        rt_taps(u, v, Ht, Wt, t);
        rt_fetch((const uint8_t*)image.data(), Wt, t, value);
        bool ok = true, back = false;
        if (mapped) {
            rt_fetch((const uint8_t*)nimage.data(), Wt, t, s);
            ok = rt_normal(s, f + 6, f + 9, nrm);
        }
        const double factor = rt_shade(cam, (int)d[0], (int)d[1], nrm, ambient, back);
        for (int k = 0; k < 4; ++k) { o[3 + k] = t.w[k]; oi[8 * q + k] = t.x[k]; oi[8 * q + 4 + k] = t.y[k]; }
        for (int k = 0; k < 3; ++k) {
            o[7 + k] = value[k]; o[10 + k] = s[k];
            albedo[k] = rt_albedo(value[k]);
            of[9 * q + k] = albedo[k]; of[9 * q + 3 + k] = nrm[k]; of[9 * q + 6 + k] = rt_lit(albedo[k], factor);
        }
        o[13] = factor; o[14] = back ? 1.0 : 0.0; o[15] = ok ? 1.0 : 0.0;
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 5;
    const bool ok = write_all(out, od) && write_all(out, oi) && write_all(out, of);
    return fclose(out) == 0 && ok ? 0 : 6;
}
