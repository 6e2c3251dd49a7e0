// Per-row cost-volume math shared by the HIP kernel and the host-side check build (tests/hostcheck).
#pragma once
#include "geom_math.h"

namespace o2345 {

struct VolGeom {
    int dx, dy, dz;
    float voxel_size, ox, oy, oz;
};

O2345_HD void voxel_xyz(long long v, const VolGeom& g, int& x, int& y, int& z) {
    z = (int)(v % g.dz);
    long long t = v / g.dz;
    y = (int)(t % g.dy);
    x = (int)(t / g.dy);
}

// number of views that see voxel (x,y,z): back_project_sparse_type(only_mask=True) summed over views
// (sparse_sdf_network.py:330-333).  coords * voxel_size + origin in fp32 (ops/back_project.py:44).
O2345_HD int visible_views(const float* __restrict__ proj, int V, int H, int W, const VolGeom& g, int x, int y, int z) {
    float wx = (float)x * g.voxel_size + g.ox, wy = (float)y * g.voxel_size + g.oy, wz = (float)z * g.voxel_size + g.oz;
    int c = 0;
    for (int i = 0; i < V; ++i) {
        float gx, gy;
        bool ok;
        project_voxel(proj + 16 * i, wx, wy, wz, H, W, gx, gy, ok);
        c += ok ? 1 : 0;
    }
    return c;
}

// One view's four bilinear taps of a channel quad (`base` = the view's map advanced by the quad, a pixel is Q float4 wide): f = sum of w * tap, then
// s1 += f, s2 += f * f.  Fully-outside taps (weight 0) are not loaded: zero padding.
template <int Q>
O2345_HD void tap4_accumulate(const float4* __restrict__ base, const int (&idx)[4], const float (&w)[4], float4& s1, float4& s2) {
    float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (w[k] != 0.f) {
            const float4 a = base[(size_t)idx[k] * Q];
            f.x += a.x * w[k]; f.y += a.y * w[k]; f.z += a.z * w[k]; f.w += a.w * w[k];
        }
    }
    s1.x += f.x; s1.y += f.y; s1.z += f.z; s1.w += f.w;
    s2.x += f.x * f.x; s2.y += f.y * f.y; s2.z += f.z * f.z; s2.w += f.w * f.w;
}

// s1, s2 over all views and the visible-view count -> var | mean of channel quad q of one output row [2 * 4Q]: mean = s1 / cnt', var = s2 / cnt' - mean^2
// with cnt' = cnt + 1e-5 (sparse_sdf_network.py:242)
template <int Q>
O2345_HD void costvol_var_mean(const float4& s1, const float4& s2, uint8_t cnt, float* __restrict__ out_row, int q) {
    const float ic = 1.f / ((float)cnt + 1e-5f);
    float4 mean = make_float4(s1.x * ic, s1.y * ic, s1.z * ic, s1.w * ic);
    float4 var = make_float4(s2.x * ic - mean.x * mean.x, s2.y * ic - mean.y * mean.y, s2.z * ic - mean.z * mean.z,
                             s2.w * ic - mean.w * mean.w);
    float4* o = reinterpret_cast<float4*>(out_row);
    o[q] = var;
    o[Q + q] = mean;
}

// One kept voxel (row), channel quad q (channels 4q..4q+3): bilinear samples of ALL views summed into
// s1 / s2, then var | mean (ops/back_project.py:44-73 fused with sparse_sdf_network.py:221-250).
template <int C>
O2345_HD void costvol_row(const float* __restrict__ feats /*[V,H,W,C]*/, const float* __restrict__ proj, int V, int H,
                          int W, const VolGeom& g, const uint8_t* __restrict__ cnt, const int* __restrict__ coords,
                          int row, int q, float* __restrict__ out /*[N,2C]*/, bool cnt_per_row = false) {
    constexpr int Q = C / 4;
    const int4 c = reinterpret_cast<const int4*>(coords)[row];
    const float wx = (float)c.x * g.voxel_size + g.ox, wy = (float)c.y * g.voxel_size + g.oy,
                wz = (float)c.z * g.voxel_size + g.oz;
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    const size_t plane = (size_t)H * W;
    for (int i = 0; i < V; ++i) {
        float gx, gy;
        bool ok;
        project_voxel(proj + 16 * i, wx, wy, wz, H, W, gx, gy, ok);
        const Taps2D tp = bilinear_taps(gx, gy, H, W);
        tap4_accumulate<Q>(reinterpret_cast<const float4*>(feats + (size_t)i * plane * C) + q, tp.idx, tp.w, s1, s2);
    }
    const long long v = ((long long)c.x * g.dy + c.y) * g.dz + c.z;
    costvol_var_mean<Q>(s1, s2, cnt[cnt_per_row ? (long long)row : v], out + (size_t)row * 2 * C, q);
}

}  // namespace o2345
