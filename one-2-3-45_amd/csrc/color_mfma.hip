// Entry points of the colour path (o2345_color_points_mfma / _x3, o2345_color_from_features, o2345_project_features: argument checks, then the launchers
// of csrc/color_pts.hip, whose k_color_pts is the kernel the product runs), and, in -DO2345_TILES_KERNEL test builds only, k_color_mfma: the same function
// (Projector.compute / compute_view_independent + GeneralRenderingNetwork.forward, models/projector.py:96-425, models/rendering_network.py:75-129)
// with another work decomposition, the independent second implementation that tests/test_gpu_parity.py::test_color_points compares against.
//
// Layer structure, both kernels: every per-(point, view) linear layer runs on the matrix cores.  Column j = lane & 31; the two wave halves
// h = lane >> 5 hold the SAME column and supply the two k rows of each MFMA step.  As in csrc/sdf_mlp.hip the MFMA result layout (neuron
// 32b + (r&3) + 8(r>>2) + 4h in register r of block b) is used as the k enumeration of the next layer, so activations stay in registers through the
// whole network; the weights are pre-permuted on the host (weights.pack_color_mfma_blob, checked lane-by-lane by tests/test_weights_packing.py).
// The 64 floats of a pixel of the channel-last map [V,H,W,64] (rgb | 56 features | pad) are split 32|32 between the halves: each lane gathers
// 8 dwordx4 per bilinear tap and owns those channels for the whole kernel.  These stages are written once, in csrc/color_net.h.
//
// Two numerical forms share everything but the matrix step (template flag X3):
//   X3 = false  v_mfma_f32_32x32x2_f32, the exact fp32 chain
//   X3 = true   split-f16 operands as in csrc/sdf_mlp_x3.hip: x = hi + lo (two f16 halves, 22 bits), products accumulated in fp32 as
//               hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16.  The per-half k enumeration is the same (register r of the fp32 form = slot 8s+t of
//               step s), so the x3 blob is a regrouping of the fp32 one (weights.pack_color_x3_blob).
//
// k_color_mfma: a wave owns 32 columns = 32/G points x G source views (G = pow2 >= V, V <= 32), every (point, view) pair is evaluated.
//   * reductions over views (min, weighted mean / variance, softmax) are DPP / xor-shuffles inside the G-lane group
//   * the view-independent rows of base_fc (geo | mean | var: 134 of 193 inputs) are evaluated once per point on the vector unit: the 2G lanes of a
//     point split the 64 outputs, exchange them through LDS, and they enter the MFMA accumulators as bias
//   * the whole blob up to the scalars (A operands, biases, the shared rows W_S: CM_TOTAL / CX_TOTAL floats, 95 / 96 KB) is staged in LDS once per
//     persistent workgroup, followed by one exchange buffer per wave
#include "color_net.h"

namespace o2345 {

// k_color_mfma is a TEST-ONLY build variant (-DO2345_TILES_KERNEL, build.build_tiles_variant()): it
// loses against k_color_pts at every view count (45.7 - 47.7 vs 36.1 - 37.0 ms at 8 views, 52.3 vs 37.1 ms at 32) and the product library does not carry it.
#ifdef O2345_TILES_KERNEL
template <int G, bool X3>
__global__ __launch_bounds__(768) void k_color_mfma(ColorMArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int PPT = 32 / G;                 // points per wave tile
    constexpr int OPV = 64 / G;                 // shared-part outputs per view lane (per half)
    constexpr int PST = 2 * 64 + 4;             // per-point stride of the exchange buffer: +4 floats so that the points of a tile map to
                                                // different LDS banks (the 32/G points read the same offsets 512 B apart otherwise)
    constexpr int SB = PPT * PST;               // floats of the per-wave exchange buffer
    constexpr int TOTAL = X3 ? CX_TOTAL : CM_TOTAL;        // floats of the staged blob
    constexpr int TAIL = X3 ? CX_A_END - CM_BIAS0 : 0;      // shift of the fp32 tail (biases, shared rows, scalars)
    for (int i = threadIdx.x * 4; i < TOTAL; i += blockDim.x * 4)
        *reinterpret_cast<float4*>(lds + i) = *reinterpret_cast<const float4*>(a.blob + i);
    __syncthreads();
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5, ptl = j / G, v = j % G;
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    float* sbuf = lds + TOTAL + wave * SB;
    const long long n = a.n_dev ? (long long)*a.n_dev : a.n;
    const float m1 = X3 ? opaque_minus_one() : -1.f;
    const float s_abs = fabsf(lds[TAIL + CM_S]) * LOG2E;
    const int base_prio = (a.sched & 1) ? (wave >> 2) : 0;          // waves w, w + 4, w + 8 share a SIMD (cyclic SIMD assignment)
    if (a.sched & 1) set_wave_prio(base_prio);
    const TileSched ts = tile_schedule(n, PPT, wave, nwave);
    for (long long tile = ts.first; tile < ts.end; tile += ts.stride) {
        const long long t0 = tile * PPT;
        const long long i = t0 + ptl;
        const bool live = i < n;
        const long long slot = live ? (a.index ? (long long)a.index[i] : i) : 0;
        const float px = live ? a.pts[3 * slot] : 0.f, py = live ? a.pts[3 * slot + 1] : 0.f, pz = live ? a.pts[3 * slot + 2] : 0.f;
        const bool view_ok = v < a.V;
        const int vv = view_ok ? v : 0;
        // ---- geometry feature (all 16 channels; needed by the shared rows) and validity ---------------------------------
        // the 8 trilinear taps are split over the view lanes of the point (G/.. lanes each load ONE 64-byte voxel), then
        // summed over the group: 4 loads per lane instead of 32 identical ones in every lane
        float geo[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) geo[c] = 0.f;
        float msum = 0.f;
        {
            // not trilinear_taps: a lane's tap number depends on its view lane, so the axis taps are picked with selects, and taps >= 8 weigh 0
            const Axis2 ax = axis_taps_zeros(px, a.D), ay = axis_taps_zeros(py, a.D), az = axis_taps_zeros(pz, a.D);
            constexpr int TPL = G >= 8 ? 1 : 8 / G;        // taps per lane
#pragma unroll
            for (int tt = 0; tt < TPL; ++tt) {
                const int tap = v * TPL + tt;               // 0..7 for v < 8/TPL; lanes beyond carry no tap
                const int ia = (tap >> 2) & 1, ib = (tap >> 1) & 1, ic = tap & 1;
                const float w = (tap < 8) ? (ia ? ax.w[1] : ax.w[0]) * (ib ? ay.w[1] : ay.w[0]) * (ic ? az.w[1] : az.w[0]) : 0.f;
                if (w != 0.f) {
                    const size_t vox = ((size_t)(ia ? ax.i[1] : ax.i[0]) * a.D + (ib ? ay.i[1] : ay.i[0])) * a.D + (ic ? az.i[1] : az.i[0]);
                    msum += w * a.maskvol[vox];
                    fma_rows<4>(reinterpret_cast<const float4*>(a.vol_cl + vox * 16), w, geo);
                }
            }
            msum = gsum<G>(msum);
#pragma unroll
            for (int c = 0; c < 16; ++c) geo[c] = gsum<G>(geo[c]);
        }
        const bool gvalid = point_valid(px, py, pz, msum);
        // geometry part of the view-independent rows right away (half 0 owns it): OPV partial sums stay live instead of 16 channels
        float sacc[OPV];
#pragma unroll
        for (int o = 0; o < OPV; ++o) sacc[o] = 0.f;
        if (h == 0) {
            const float* WG = lds + TAIL + CM_W_S + v * OPV;
#pragma unroll
            for (int c = 0; c < 16; ++c)
#pragma unroll
                for (int o = 0; o < OPV; ++o) sacc[o] = fmaf(geo[c], WG[c * 64 + o], sacc[o]);
        }
        // ---- this lane's view: projection, mask, ray direction difference; this half's 32 pixel floats + ray_dir_fc ---------------------
        float qx, qy, qz;
        query_direction(a.normals, a.query_cam, slot, px, py, pz, qx, qy, qz);
        const ViewGeom g = view_geom(a, vv, px, py, pz, qx, qy, qz, gvalid && view_ok, s_abs);
        const float m = g.m;
        float rf[32];
        if (a.sched & 2) set_wave_prio(3);
        gather_now(a, h, vv, g, rf);
        if (a.sched & 2) set_wave_prio(base_prio);
        const float rgb0 = rf[0], rgb1 = rf[1], rgb2 = rf[2];      // log2(e) * colours (meaningful in half 0), before the direction feature
        add_direction_feature<X3>(lds, TAIL, lane, h, g.rd, m1, rf);
        // ---- pooling weights over views ----------------------------------------------------------------------------------------------
        const float emin = gmin<G>(view_ok ? g.e : INFINITY);
        float wgt = (g.e - emin) * m;
        wgt = wgt * crcp(gsum<G>(wgt) + 1e-8f);
        // ---- view-independent rows: this lane's OPV outputs over its half's channels -------------------------------------------------
        {
            const float* WS = lds + TAIL + CM_W_S + v * OPV;
            const float* WM = WS + (16 + 32 * h) * 64;
            const float* WV = WS + (80 + 32 * h) * 64;
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                const float mean = gsum<G>(rf[c] * wgt);
                const float dd = rf[c] - mean;
                const float var = gsum<G>(wgt * dd * dd);
#pragma unroll
                for (int o = 0; o < OPV; ++o) sacc[o] = fmaf(var, WV[c * 64 + o], fmaf(mean, WM[c * 64 + o], sacc[o]));
            }
            float* sb = sbuf + ptl * PST + h * 64 + v * OPV;
#pragma unroll
            for (int o = 0; o < OPV; ++o) sb[o] = sacc[o];
            __builtin_amdgcn_wave_barrier();
        }
        // ---- the per-view network on top of bias + exchanged shared rows ---------------------------------------------------------------
        f32x16 acc[2];
        cm_bias<2>(acc, lds + TAIL + CM_B_B0, h);
        {
            const float* s0 = sbuf + ptl * PST;
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int nidx = 32 * b + (r & 3) + 8 * (r >> 2) + 4 * h;
                    acc[b][r] += s0[nidx] + s0[64 + nidx];
                }
            __builtin_amdgcn_wave_barrier();
        }
        float score = view_network<X3>(acc, rf, g.rd, wgt, m, m1, lds, TAIL, lds + TAIL + CM_S, lane, h);
        // ---- masked softmax over views, blended colour ----------------------------------------------------------------------------------
        if (m == 0.f) score = -1e9f;
        if (!view_ok) score = -INFINITY;
        const float smax = gmax<G>(score);
        const float ex = view_ok ? __builtin_amdgcn_exp2f(score - smax) : 0.f;      // scores are in the scaled domain
        const float bw = ex * crcp(gsum<G>(ex));
        const float bwn = bw * LN2;                                 // undo the scale of the colours
        const float c0 = gsum<G>(rgb0 * bwn), c1 = gsum<G>(rgb1 * bwn), c2 = gsum<G>(rgb2 * bwn);
        const float nv = gsum<G>(m);
        if (live && v == 0 && h == 0) {
            a.out_rgb[3 * slot] = c0; a.out_rgb[3 * slot + 1] = c1; a.out_rgb[3 * slot + 2] = c2;
            if (a.out_nviews) a.out_nviews[slot] = (uint8_t)(nv + 0.5f);
        }
    }
}

#endif  // O2345_TILES_KERNEL

}  // namespace o2345

using namespace o2345;

extern "C" {

int o2345_color_mfma_blob_floats(void) { return CM_TOTAL2; }
int o2345_color_x3_blob_floats(void) { return CX_TOTAL2; }

// both numerical forms of o2345_color_points_*: x3 = 1 takes the blob of weights.pack_color_x3_blob (o2345_color_x3_blob_floats() floats), 0 that of
// weights.pack_color_mfma_blob
}  // extern "C"

int o2345::color_points_launch(int x3, const float* blob, const float* vol_cl, const float* maskvol, int D, const float* cmaps, const float* proj,
                               const float* cam_pos, int V, int H, int W, const float* pts, const int32_t* index, const int32_t* n_dev, long long n,
                               const float* query_cam, const float* normals, float* out_rgb, uint8_t* out_nviews, unsigned long long* stats_dev,
                               int32_t* tile_queue, void* stream) {
    O2345_REQUIRE(blob && vol_cl && maskvol && cmaps && proj && cam_pos && pts && out_rgb, "color_points: null pointer");
    O2345_REQUIRE((query_cam != nullptr) != (normals != nullptr), "color_points: give exactly one of query_cam / normals");
    O2345_REQUIRE(V >= 1 && V <= 255, "color_points: V must be in [1,255] (valid-view counts are stored as uint8; got %d)", V);
    if (n <= 0 && !n_dev) return 0;
    O2345_REQUIRE(!tile_queue || n <= TQ_MAX_TILES * 32, "color_points: a tile queue indexes at most %lld tiles", TQ_MAX_TILES);
    ColorMArgs a{blob, vol_cl, maskvol, D, cmaps, proj, cam_pos, V, H, W, pts, index, n_dev, n, query_cam, normals, out_rgb, out_nviews};
    a.sched = color_sched_mode();
    a.stats = stats_dev;                         // optional, caller-owned work counters [4] (k_color_pts only)
    a.tile_queue = tile_queue;                   // optional, zero at launch (k_color_pts only)
#ifdef O2345_TILES_KERNEL
    // test-only variant: O2345_COLOR_KERNEL=tiles selects k_color_mfma (columns = (point, view) pairs, view count padded to a power of two <= 32, every
    // pair evaluated) -- the A/B partner of k_color_pts in tests/test_gpu_parity.py::test_color_points and tests/test_gpu_edges_and_fullsize.py
    if (knobs().color_tiles && V <= 32) {
        int G = 4;
        while (G < V) G <<= 1;
        const int threads = 768, ppt = 32 / G;
        const unsigned grid = network_grid(n, n_dev, threads, ppt);
        const size_t lds = (size_t)((x3 ? CX_TOTAL : CM_TOTAL) + (threads / 64) * ppt * (2 * 64 + 4)) * sizeof(float);
        hipStream_t s = (hipStream_t)stream;
#define O2345_CM_CASE(GG, XX)                                                                                              \
    if (G == GG && (x3 != 0) == XX) {                                                                                      \
        O2345_ENSURE_LDS((k_color_mfma<GG, XX>), lds);                                                                     \
        hipLaunchKernelGGL((k_color_mfma<GG, XX>), dim3(grid), dim3(threads), lds, s, a);                                  \
    }
        O2345_CM_CASE(4, false) O2345_CM_CASE(8, false) O2345_CM_CASE(16, false) O2345_CM_CASE(32, false)
        O2345_CM_CASE(4, true) O2345_CM_CASE(8, true) O2345_CM_CASE(16, true) O2345_CM_CASE(32, true)
#undef O2345_CM_CASE
        return check_launch("color_points (tiles kernel)");
    }
#endif
    return color_pts_launch(a, x3, false, "color_points (points-as-columns kernel)", stream);
}

extern "C" {

// the _q forms: the tail of the tile list goes through `tile_queue` (8 ints of caller memory, cleared here on the launch stream)
static int color_points_q(int x3, const float* blob, const float* vol_cl, const float* maskvol, int D, const float* cmaps, const float* proj,
                          const float* cam_pos, int V, int H, int W, const float* pts, const int32_t* index, const int32_t* n_dev, long long n,
                          const float* query_cam, const float* normals, float* out_rgb, uint8_t* out_nviews, unsigned long long* stats_dev,
                          int32_t* tile_queue, void* stream) {
    O2345_REQUIRE(tile_queue, "color_points_q: null tile queue");
    O2345_HIP(hipMemsetAsync(tile_queue, 0, TQ_HEADS * sizeof(int32_t), (hipStream_t)stream));
    return color_points_launch(x3, blob, vol_cl, maskvol, D, cmaps, proj, cam_pos, V, H, W, pts, index, n_dev, n, query_cam, normals, out_rgb, out_nviews, stats_dev,
                               tile_queue, stream);
}
int o2345_color_points_x3_q(const float* blob, const float* vol_cl, const float* maskvol, int D, const float* cmaps,
                            const float* proj, const float* cam_pos, int V, int H, int W, const float* pts,
                            const int32_t* index, const int32_t* n_dev, long long n, const float* query_cam,
                            const float* normals, float* out_rgb, uint8_t* out_nviews, unsigned long long* stats_dev, int32_t* tile_queue, void* stream) {
    return color_points_q(1, blob, vol_cl, maskvol, D, cmaps, proj, cam_pos, V, H, W, pts, index, n_dev, n, query_cam, normals, out_rgb, out_nviews, stats_dev,
                          tile_queue, stream);
}
int o2345_color_points_mfma_q(const float* blob, const float* vol_cl, const float* maskvol, int D, const float* cmaps,
                              const float* proj, const float* cam_pos, int V, int H, int W, const float* pts,
                              const int32_t* index, const int32_t* n_dev, long long n, const float* query_cam,
                              const float* normals, float* out_rgb, uint8_t* out_nviews, unsigned long long* stats_dev, int32_t* tile_queue, void* stream) {
    return color_points_q(0, blob, vol_cl, maskvol, D, cmaps, proj, cam_pos, V, H, W, pts, index, n_dev, n, query_cam, normals, out_rgb, out_nviews, stats_dev,
                          tile_queue, stream);
}

int o2345_color_points_mfma(const float* blob, const float* vol_cl, const float* maskvol, int D, const float* cmaps,
                            const float* proj, const float* cam_pos, int V, int H, int W, const float* pts,
                            const int32_t* index, const int32_t* n_dev, long long n, const float* query_cam,
                            const float* normals, float* out_rgb, uint8_t* out_nviews, unsigned long long* stats_dev, void* stream) {
    return color_points_launch(0, blob, vol_cl, maskvol, D, cmaps, proj, cam_pos, V, H, W, pts, index, n_dev, n, query_cam, normals, out_rgb, out_nviews, stats_dev, nullptr, stream);
}
int o2345_color_points_x3(const float* blob, const float* vol_cl, const float* maskvol, int D, const float* cmaps,
                          const float* proj, const float* cam_pos, int V, int H, int W, const float* pts,
                          const int32_t* index, const int32_t* n_dev, long long n, const float* query_cam,
                          const float* normals, float* out_rgb, uint8_t* out_nviews, unsigned long long* stats_dev, void* stream) {
    return color_points_launch(1, blob, vol_cl, maskvol, D, cmaps, proj, cam_pos, V, H, W, pts, index, n_dev, n, query_cam, normals, out_rgb, out_nviews, stats_dev, nullptr, stream);
}

// Projector.compute (query_cam) / compute_view_independent (normals) materialised: geometry_feat [P,16], rgb_feat [V,P,59], ray_diff [V,P,4],
// mask [V,P] (1 / 0) in the reference's view-major layout (models/projector.py:96-425)
int o2345_project_features(const float* vol_cl, const float* maskvol, int D, const float* cmaps, const float* proj, const float* cam_pos, int V, int H,
                           int W, const float* pts, long long P, const float* query_cam, const float* normals, float* geometry_feat, float* rgb_feat,
                           float* ray_diff, float* mask, void* stream) {
    O2345_REQUIRE(vol_cl && maskvol && cmaps && proj && cam_pos && pts && geometry_feat && rgb_feat && ray_diff && mask, "project_features: null pointer");
    O2345_REQUIRE((query_cam != nullptr) != (normals != nullptr), "project_features: give exactly one of query_cam / normals");
    O2345_REQUIRE(V >= 1 && V <= 255 && P >= 0 && P * V < (1ll << 33), "project_features: bad sizes (V in [1,255])");
    if (P == 0) return 0;
    const ColorMArgs a{nullptr, vol_cl, maskvol, D, cmaps, proj, cam_pos, V, H, W, pts, nullptr, nullptr, P, query_cam, normals, nullptr, nullptr};
    return project_features_launch(a, geometry_feat, rgb_feat, ray_diff, mask, stream);
}

// GeneralRenderingNetwork.forward(geometry_feat, rgb_feat, ray_diff, mask) on materialised tensors in the reference's layout (view-major):
// geometry_feat [P,16], rgb_feat [V,P,59], ray_diff [V,P,4], mask [V,P] (non-zero = valid) -> rgb [P,3], number of valid views [P].
// x3 = 1: blob from weights.pack_color_x3_blob (split-f16 form), 0: weights.pack_color_mfma_blob (fp32 MFMA).
int o2345_color_from_features(const float* blob, int x3, const float* geometry_feat, const float* rgb_feat, const float* ray_diff, const float* mask,
                              int V, long long P, float* out_rgb, uint8_t* out_nviews, void* stream) {
    O2345_REQUIRE(blob && geometry_feat && rgb_feat && ray_diff && mask && out_rgb, "color_from_features: null pointer");
    O2345_REQUIRE(V >= 1 && V <= 255 && P >= 0, "color_from_features: bad sizes (V in [1,255]: valid-view counts are stored as uint8)");
    if (P == 0) return 0;
    ColorMArgs a{};                              // sched stays 0: this form runs without the O2345_COLOR_SCHED knobs
    a.blob = blob; a.V = V; a.n = P; a.out_rgb = out_rgb; a.out_nviews = out_nviews;
    a.f_geo = geometry_feat; a.f_rgb = rgb_feat; a.f_rdiff = ray_diff; a.f_mask = mask;
    return color_pts_launch(a, x3, true, "color_from_features", stream);
}

}  // extern "C"
