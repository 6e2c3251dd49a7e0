// Image-based colour blending, "points as columns" form: the same function as csrc/color_mfma.hip
// (Projector.compute / compute_view_independent + GeneralRenderingNetwork.forward, models/projector.py:96-425,
// models/rendering_network.py:75-129) with a different work decomposition.
//
// csrc/color_mfma.hip makes a (point, view) pair a matrix column, so everything that couples the views of a point -- pooling
// weights, weighted mean / variance of 64 pixel floats, the view-independent rows of base_fc.0, the final softmax -- crosses
// lanes: 236 DPP adds (6.3 cycles each on gfx950), 320 packed FMAs on 128 KB of LDS weight rows and an LDS exchange per 4 points.
// On this chip a SIMD issues EITHER vector OR matrix work (profiles/r02_ubench_issue_model.md), so that vector work is not hidden.
//
// Here a wave owns 32 POINTS (column j = lane & 31, the two halves h = lane >> 5 own 32 of the 64 pixel floats each, as before)
// and walks the V source views in three passes, keeping every per-point quantity in registers of the point's two lanes:
//   pass 0   geometry feature (8 channels per half), validity, query direction, min over views of the pooling exponent;
//   pass A   per view: bilinear gather of the half pixel, ray_dir_fc (4 -> 16 -> 59, matrix cores), weighted running mean and
//            M2 of the 32 pixel floats (Welford update with the un-normalised pooling weights: no cross-lane traffic, no cancellation);
//   shared   view-independent rows of base_fc.0 (geo | mean | var -> 64) ONCE per point on the matrix cores (N = 32 points): the
//            result (incl. bias) is the accumulator input of every view's base_fc.0;
//   pass B   per view: gather + ray_dir_fc again (recomputed: 59 floats x V per point do not fit anywhere), base_fc, vis_fc,
//            vis_fc2, rgb_fc (view_network of color_net.h, the function k_color_mfma calls), and an online softmax over the views
//            (running max / sum / rgb).
// View-uniform data (projection rows, camera centres) is read through scalar loads.  V is a run-time loop bound: no power-of-two
// padding of the view count, any V >= 1.  LDS holds the operand blobs (without A_S) and one slot of shared rows per wave (<= 148 KB).
#include "color_net.h"

namespace o2345 {

// FEATS form (GeneralRenderingNetwork.forward on materialised tensors, rendering_network.py:75-129): the same per-view quantities read from the
// reference's view-major inputs instead of being derived from the point
__device__ __forceinline__ ViewGeom feat_geom(const ColorMArgs& a, int v, long long slot, float s_abs) {
    ViewGeom g;
    const float4 rd = *reinterpret_cast<const float4*>(a.f_rdiff + ((size_t)v * a.n + slot) * 4);
    g.rd[0] = rd.x; g.rd[1] = rd.y; g.rd[2] = rd.z; g.rd[3] = rd.w;
    g.e = __builtin_amdgcn_exp2f(s_abs * (rd.w - 1.f));
    g.m = a.f_mask[(size_t)v * a.n + slot] != 0.f ? 1.f : 0.f;
    g.gx = g.gy = 0.f;
    return g;
}
__device__ __forceinline__ void load_feats(const ColorMArgs& a, int h, int v, long long slot, float (&rf)[32]) {
    const float* src = a.f_rgb + ((size_t)v * a.n + slot) * 59 + 32 * h;
#pragma unroll
    for (int c = 0; c < 32; ++c) rf[c] = (h == 0 || c < 27) ? src[(h == 0 || c < 27) ? c : 0] * LOG2E : 0.f;
}

// this half's 32 pixel floats of view v, before the direction feature: read (FEATS) or gathered with the wave's priority raised (bit 1 of a.sched)
template <bool FEATS>
__device__ __forceinline__ void pixel_floats(const ColorMArgs& a, int h, int v, long long slot, const ViewGeom& g, int base_prio, float (&rf)[32]) {
    if constexpr (FEATS) load_feats(a, h, v, slot, rf);
    else {
        if (a.sched & 2) set_wave_prio(3);
        gather_now(a, h, v, g, rf);
        if (a.sched & 2) set_wave_prio(base_prio);
    }
}

// The view-independent rows of base_fc.0 (A_S, 36 KB in either form, read once per tile) come straight from the blob in global memory, where they stay
// L2-resident: not staging them leaves the LDS room for the per-wave slots of their result (below).  They are read through a buffer descriptor: the k-step
// offsets go to the scalar offset operand (64-bit per-load addresses cost 72 VGPRs, hoisted out of the tile loop).  The next k-step's operands are
// requested before this step's matrix work (an L2 hit takes about as long as one step's matrix instructions).  Same operations in the same order as
// cx_run / cm_run.
constexpr int CP_AS_BYTES = 2 * 9 * 512 * 4;                              // == 2 * 72 * 64 * 4 (fp32 form)
template <int NB, int N>
__device__ __forceinline__ void cx_run_global(f32x16 (&acc)[NB], __amdgpu_buffer_rsrc_t rs, int lane, const float (&b)[N], float m1) {
    constexpr int NS = (N + 7) / 8;
    auto fetch = [&](int nb, int s, int k) { return __builtin_bit_cast(h16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, ((nb * NS + s) * 2 + k) * 1024, 0)); };
    h16x8 cur[NB][2], nxt[NB][2];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { cur[nb][0] = fetch(nb, 0, 0); cur[nb][1] = fetch(nb, 0, 1); }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s + 1 < NS) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) { nxt[nb][0] = fetch(nb, s + 1, 0); nxt[nb][1] = fetch(nb, s + 1, 1); }
        }
        const Split8 sp = split8(b, 8 * s, m1);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = MFMA_F16(cur[nb][1], sp.hi, acc[nb]);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = MFMA_F16(cur[nb][0], sp.lo, acc[nb]);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = MFMA_F16(cur[nb][0], sp.hi, acc[nb]);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) { cur[nb][0] = nxt[nb][0]; cur[nb][1] = nxt[nb][1]; }
        __builtin_amdgcn_sched_barrier(0);
    }
}
template <int NB, int N>
__device__ __forceinline__ void cm_run_global(f32x16 (&acc)[NB], __amdgpu_buffer_rsrc_t rs, int lane, const float (&b)[N]) {
    auto fetch = [&](int nb, int r) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, lane * 4, (nb * N + r) * 256, 0)); };
    float cur[NB], nxt[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) cur[nb] = fetch(nb, 0);
#pragma unroll
    for (int r = 0; r < N; ++r) {
        if (r + 1 < N) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) nxt[nb] = fetch(nb, r + 1);
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = MFMA32(cur[nb], b[r], acc[nb]);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) cur[nb] = nxt[nb];
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Those rows' result (incl. bias: 2 accumulator blocks = 32 floats per lane) is the starting accumulator of every view's base_fc.0 in pass B.  It waits in
// an 8 KB LDS slot per wave, [block][quarter][64 lanes][4 floats] (conflict-free 16-byte accesses), instead of 32 registers live through pass B: that is
// what brings the kernel under 168 VGPRs, i.e. 3 waves per SIMD.  Each lane reads back only what it wrote: no barrier.
__device__ __forceinline__ void sh_store(float4* slot, const f32x16 (&sh)[2]) {
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q) slot[(nb * 4 + q) * 64] = make_float4(sh[nb][4 * q], sh[nb][4 * q + 1], sh[nb][4 * q + 2], sh[nb][4 * q + 3]);
}
__device__ __forceinline__ void sh_load(f32x16 (&acc)[2], const float4* slot) {
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 t = slot[(nb * 4 + q) * 64];
            acc[nb][4 * q] = t.x; acc[nb][4 * q + 1] = t.y; acc[nb][4 * q + 2] = t.z; acc[nb][4 * q + 3] = t.w;
        }
}

// 768-thread workgroups: 3 waves per SIMD, <= 168 VGPRs.  Nothing spills inside a view loop; the f16x3 forms keep a few tile-level values (indices,
// addresses) in scratch.  (Earlier forms: 512 threads at 199 VGPRs; a 768-thread build that kept the shared rows in registers spilled 140 B and lost,
// 46.0 vs 45.2 ms.)
constexpr int CP_THREADS = 768;
// tile queue (a.tile_queue): share of the tile list that is claimed instead of dealt, 1 / 2^shift (0: all of it), and tiles per claim (a tile is about
// 37 us: a claim's latency is noise).  Measured at 1/16, 1/8, 1/4, 1/2 and everything: the more is claimed the faster (profiles/NOTES.md, round 11) --
// every wave starts at its XCD's head, so an XCD still works through one contiguous eighth of the list and then helps the others.
#ifndef O2345_CP_TQ_SHARE_SHIFT
#define O2345_CP_TQ_SHARE_SHIFT 0
#endif
constexpr int CP_TQ_SHARE_SHIFT = O2345_CP_TQ_SHARE_SHIFT, CP_TQ_CLAIM = 1;
constexpr int CP_SH_FLOATS = 2 * 16 * 64;                                  // one wave's slot of shared rows
// dynamic LDS: [A segments | biases and per-lane vectors] [scalars (4)] [one shared-row slot per wave]
constexpr size_t color_pts_lds_bytes(int x3) {
    return (size_t)((x3 ? CX_A_END + CM_W_S - CM_BIAS0 : CM_W_S) + 4 + (CP_THREADS / 64) * CP_SH_FLOATS) * sizeof(float);
}
static_assert(color_pts_lds_bytes(1) <= 160 * 1024 && color_pts_lds_bytes(0) <= 160 * 1024, "k_color_pts: LDS of a CU exceeded");
template <bool X3, bool FEATS>
__global__ __launch_bounds__(CP_THREADS) void k_color_pts(ColorMArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // staged: [A segments | biases and per-lane vectors] [scalars (4)]  -- the VALU weight rows W_S of color_mfma.hip are skipped, A_S is read from global memory
    constexpr int HEAD = X3 ? (CX_A_END + CM_W_S - CM_BIAS0) : CM_W_S;       // floats before W_S in the blob
    constexpr int SRC_S = X3 ? (CX_TOTAL - 4) : CM_S;                       // scalars in the blob
    constexpr int TAIL = X3 ? CX_A_END - CM_BIAS0 : 0;                      // shift of the bias block, as in color_mfma.hip
    constexpr int L_S = HEAD, L_SH = HEAD + 4;                              // LDS offsets of the scalars and of the shared-row slots
    for (int i = threadIdx.x * 4; i < HEAD; i += blockDim.x * 4)
        *reinterpret_cast<float4*>(lds + i) = *reinterpret_cast<const float4*>(a.blob + i);
    if (threadIdx.x == 0) *reinterpret_cast<float4*>(lds + L_S) = *reinterpret_cast<const float4*>(a.blob + SRC_S);
    __syncthreads();
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    float4* const sh_slot = reinterpret_cast<float4*>(lds + L_SH + wave * CP_SH_FLOATS) + lane;
    const long long n = a.n_dev ? (long long)*a.n_dev : a.n;
    const float m1 = X3 ? opaque_minus_one() : -1.f;
    const float s_abs = fabsf(lds[L_S]) * LOG2E;
    const int V = a.V;
    const bool skip_views = V <= 64 && !(a.sched & 4);              // bit 2 of O2345_COLOR_SCHED: evaluate every view (A/B runs)
    const bool skip_zero = skip_views && !(a.sched & 16);           // bit 4: evaluate zero-weight pooling views in pass A
    const int base_prio = (a.sched & 1) ? (wave >> 2) : 0;          // waves w, w + 4 and w + 8 share a SIMD (cyclic SIMD assignment over 4 SIMDs)
    if (a.sched & 1) set_wave_prio(base_prio);
    // bit 3 of O2345_COLOR_SCHED: block-interleaved tiles instead of one contiguous eighth of the list per XCD (A/B: with view skipping the
    // cost of a tile depends on where its rays look, and a contiguous eighth of the image is not an eighth of the work).  With a tile queue the last
    // 1 / 2^CP_TQ_SHARE_SHIFT of the list is not dealt but claimed, CP_TQ_CLAIM tiles at a time (common.h; profiles/NOTES.md round 11 has the arms).
    const TileQueue tq = tile_queue_split((n + 31) / 32, (long long)gridDim.x * nwave, CP_TQ_SHARE_SHIFT, a.tile_queue != nullptr);
    const TileSched ts = (a.sched & 8) ? tile_schedule_flat_at(tq.n_static, blockIdx.x, gridDim.x, wave, nwave) : tile_schedule_tiles(tq.n_static, wave, nwave);
    const auto static_end = [&](long long n_static) { return (a.sched & 8) ? n_static : tile_schedule_tiles(n_static, wave, nwave).end; };
    TileCursor cur;
    unsigned st_a = 0, st_b = 0, st_t = 0, st_full = 0;          // wave-uniform work counters (a.stats)
    for (long long tile = tile_first<CP_TQ_CLAIM>(cur, ts, tq, a.tile_queue); tile >= 0; tile = tile_next<CP_TQ_CLAIM>(cur, tile, (n + 31) / 32, a.tile_queue, static_end)) {
        const long long i = tile * 32 + j;
        const bool live = i < n;
        const long long slot = live ? (a.index ? (long long)a.index[i] : i) : 0;
        const float px = (live && !FEATS) ? a.pts[3 * slot] : 0.f, py = (live && !FEATS) ? a.pts[3 * slot + 1] : 0.f,
                    pz = (live && !FEATS) ? a.pts[3 * slot + 2] : 0.f;
        // ---- pass 0: geometry feature (this half's 8 channels), validity, query direction ---------------------------------------
        float bs[72];                               // per-half operands of the shared rows: geo (8) | mean (32) | var (32)
        bool gvalid;
        if constexpr (FEATS) {
            const float4* g4 = reinterpret_cast<const float4*>(a.f_geo + (size_t)slot * 16) + 2 * h;
            const float4 t0 = g4[0], t1 = g4[1];
            bs[0] = t0.x; bs[1] = t0.y; bs[2] = t0.z; bs[3] = t0.w; bs[4] = t1.x; bs[5] = t1.y; bs[6] = t1.z; bs[7] = t1.w;
            gvalid = true;
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) bs[c] = 0.f;
            const float msum = trilinear_taps(px, py, pz, a.D, a.maskvol, [&](size_t vox, float w) {
                fma_rows<2>(reinterpret_cast<const float4*>(a.vol_cl + vox * 16) + 2 * h, w, bs);
            });
            gvalid = point_valid(px, py, pz, msum);
        }
        float qx = 0.f, qy = 0.f, qz = 0.f;
        if constexpr (!FEATS) query_direction(a.normals, a.query_cam, slot, px, py, pz, qx, qy, qz);
        // min over ALL views of the pooling exponent (rendering_network.py:94: exp(...).min over the view axis, mask or not)
        float emin = INFINITY;
        for (int v = 0; v < V; ++v) {
            if constexpr (FEATS) {
                emin = fminf(emin, __builtin_amdgcn_exp2f(s_abs * (a.f_rdiff[((size_t)v * a.n + slot) * 4 + 3] - 1.f)));
                continue;
            }
            const float sx = a.cam_pos[3 * v] - px, sy = a.cam_pos[3 * v + 1] - py, sz = a.cam_pos[3 * v + 2] - pz;
            const float rsn = crcp(sqrtf(sx * sx + sy * sy + sz * sz) + 1e-6f);
            const float dot = qx * (sx * rsn) + qy * (sy * rsn) + qz * (sz * rsn);
            emin = fminf(emin, __builtin_amdgcn_exp2f(s_abs * (dot - 1.f)));
        }
        // ---- pass A: weighted mean / variance over the views of this half's 32 pixel floats ----------------------------------------
        // Welford update with the un-normalised weights raw_v = (e_v - emin) m_v: mean_w = sum(raw x)/sum(raw), M2 = sum raw (x - mean_w)^2
        float wsum = 0.f, nvis = 0.f;
        unsigned long long active = 0ull;            // wave-uniform: views that see at least one point of the tile
        {
            // M2 waits in this wave's shared-row slot (free until the shared rows), read and written back once per evaluated view: 32 registers
            // fewer in pass A.  `fresh` (wave-uniform): no view evaluated yet, M2 = 0.
            float mean[32];
#pragma unroll
            for (int c = 0; c < 32; ++c) mean[c] = 0.f;
            bool fresh = true;
#pragma unroll 1
            for (int v = 0; v < V; ++v) {
                asm volatile("" ::: "memory");              // keeps M2 in the LDS (no promotion of the slot to registers across the view loop)
                const ViewGeom g = FEATS ? feat_geom(a, v, slot, s_abs) : view_geom(a, v, px, py, pz, qx, qy, qz, gvalid, s_abs);
                // A view that sees NONE of the tile's 32 points (wave-uniform test) contributes exactly nothing to this pass: raw = 0 leaves wsum,
                // nvis, mean and M2 bit-unchanged.  Points of a tile are neighbours (32 adjacent rays at one sample index), so visibility is
                // coherent: at BASELINE config 2 a point is seen by 4.8 of the 8 views on average and 37 % of the (tile, view) pairs are skipped.
                if (skip_views && __builtin_amdgcn_ballot_w64(g.m != 0.f) == 0ull) continue;
                active |= 1ull << (v & 63);                  // pass B evaluates the view
                const float raw = (g.e - emin) * g.m;
                nvis += g.m;
                // The same holds for a view that the tile's points see, but all with pooling weight raw = 0: emin comes from exactly the operations
                // that give g.e (same dot product, same exp2, no contraction), so for every point its view of smallest e has raw = 0 exactly, and
                // neighbouring points share that view.  Such a view leaves wsum, mean and M2 bit-unchanged; it still counts in nvis and in pass B.
                if (skip_zero && __builtin_amdgcn_ballot_w64(live && raw != 0.f) == 0ull) continue;
                ++st_a;
                float rf[32];
                pixel_floats<FEATS>(a, h, v, slot, g, base_prio, rf);
                add_direction_feature<X3>(lds, TAIL, lane, h, g.rd, m1, rf);
                wsum += raw;
                const float r0 = raw > 0.f ? raw * crcp(wsum) : 0.f;
                // one Newton step on the quotient: raw / wsum to <= 1 ulp
                const float rq = raw > 0.f ? fmaf(fmaf(-wsum, r0, raw), crcp(wsum), r0) : 0.f;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    float4 t = fresh ? make_float4(0.f, 0.f, 0.f, 0.f) : sh_slot[q * 64];
                    float* m2 = reinterpret_cast<float*>(&t);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int c = 4 * q + k;
                        const float d = rf[c] - mean[c];
                        mean[c] = fmaf(rq, d, mean[c]);
                        m2[k] = fmaf(raw * d, rf[c] - mean[c], m2[k]);
                    }
                    sh_slot[q * 64] = t;
                }
                fresh = false;
            }
            // the reference normalises the weights by (sum + 1e-8): w_v = raw_v / (wsum + 1e-8), S = sum w_v <= 1
            //   mean_ref = sum w x = S mean_w,   var_ref = sum w (x - mean_ref)^2 = M2 / (wsum + 1e-8) + S (1 - S)^2 mean_w^2
            const float rden = crcp(wsum + 1e-8f);
            const float S = wsum * rden, k2 = S * (1.f - S) * (1.f - S);
            asm volatile("" ::: "memory");
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 t = fresh ? make_float4(0.f, 0.f, 0.f, 0.f) : sh_slot[q * 64];
                const float m2[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = 4 * q + k;
                    bs[8 + c] = S * mean[c];
                    bs[40 + c] = fmaf(k2 * mean[c], mean[c], m2[k] * rden);
                }
            }
        }
        const float rden = crcp(wsum + 1e-8f);
        // ---- view-independent rows of base_fc.0, once per point: sh = bias + W_shared [geo | mean | var] -------------------------
        {
            f32x16 sh[2];
            cm_bias<2>(sh, lds + TAIL + CM_B_B0, h);
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.blob + (X3 ? CX_A_S : CM_A_S)), 0, CP_AS_BYTES, 0x00020000);
            if constexpr (X3) cx_run_global<2, 72>(sh, rs, lane, bs, m1);
            else cm_run_global<2, 72>(sh, rs, lane, bs);
            sh_store(sh_slot, sh);
        }
        // ---- pass B: per view network, online softmax over the views ------------------------------------------------------------------
        float smax = -INFINITY, ssum = 0.f, o0 = 0.f, o1 = 0.f, o2 = 0.f;
        // A masked view enters the softmax with score -1e9: its blending weight is exp2(-1e9 - max) = 0 EXACTLY as soon as the point has one
        // visible view, whatever the order.  Only a point with NO visible view blends the masked views (uniformly): if the tile holds such a
        // point, every view is evaluated as before; otherwise the views that see none of the tile's points are skipped -- bit-identical results.
        const bool skip_b = skip_views && __builtin_amdgcn_ballot_w64(live && nvis == 0.f) == 0ull;
        ++st_t;
        st_full += skip_b ? 0u : 1u;
#pragma unroll 1
        for (int v = 0; v < V; ++v) {
            if (skip_b && !((active >> (v & 63)) & 1ull)) continue;
            ++st_b;
            const ViewGeom g = FEATS ? feat_geom(a, v, slot, s_abs) : view_geom(a, v, px, py, pz, qx, qy, qz, gvalid, s_abs);
            const float m = g.m;
            float rf[32];
            pixel_floats<FEATS>(a, h, v, slot, g, base_prio, rf);
            const float rgb0 = rf[0], rgb1 = rf[1], rgb2 = rf[2];   // log2(e) * colours (meaningful in half 0), before the direction feature
            add_direction_feature<X3>(lds, TAIL, lane, h, g.rd, m1, rf);
            // ---- base_fc (on top of the shared rows), vis_fc, vis_fc2, rgb_fc
            f32x16 acc[2];
            sh_load(acc, sh_slot);
            float score = view_network<X3>(acc, rf, g.rd, (g.e - emin) * m * rden, m, m1, lds, TAIL, lds + L_S, lane, h);
            // ---- masked softmax over the views, running form (scores are in the scaled domain: base 2)
            if (m == 0.f) score = -1e9f;
            const float nmax = fmaxf(smax, score);
            const float sc_old = __builtin_amdgcn_exp2f(smax - nmax), ex = __builtin_amdgcn_exp2f(score - nmax);
            ssum = fmaf(ssum, sc_old, ex);
            o0 = fmaf(o0, sc_old, ex * rgb0); o1 = fmaf(o1, sc_old, ex * rgb1); o2 = fmaf(o2, sc_old, ex * rgb2);
            smax = nmax;
        }
        if (live && h == 0) {
            const float rs = crcp(ssum) * LN2;                       // undo the scale of the colours
            a.out_rgb[3 * slot] = o0 * rs; a.out_rgb[3 * slot + 1] = o1 * rs; a.out_rgb[3 * slot + 2] = o2 * rs;
            if (a.out_nviews) a.out_nviews[slot] = (uint8_t)(nvis + 0.5f);
        }
    }
    if (a.stats && lane == 0) {
        atomicAdd(a.stats + 0, (unsigned long long)st_a); atomicAdd(a.stats + 1, (unsigned long long)st_b);
        atomicAdd(a.stats + 2, (unsigned long long)st_t); atomicAdd(a.stats + 3, (unsigned long long)st_full);
    }
}

// One launch of k_color_pts.  x3: the split-f16 form and its blob; feats: GeneralRenderingNetwork.forward on the reference's materialised tensors
// a.f_* (the drop-in form) instead of the fused Projector path, which is the fast one.
template <auto KERNEL>
static int color_pts_launch_kernel(const ColorMArgs& a, size_t lds, const char* what, void* stream) {
    O2345_ENSURE_LDS(KERNEL, lds);
    hipLaunchKernelGGL(KERNEL, dim3(network_grid(a.n, a.n_dev, CP_THREADS, 32)), dim3(CP_THREADS), lds, (hipStream_t)stream, a);
    return check_launch(what);
}
int color_pts_launch(const ColorMArgs& a, int x3, bool feats, const char* what, void* stream) {
    const auto launch = x3 ? (feats ? color_pts_launch_kernel<k_color_pts<true, true>> : color_pts_launch_kernel<k_color_pts<true, false>>)
                           : (feats ? color_pts_launch_kernel<k_color_pts<false, true>> : color_pts_launch_kernel<k_color_pts<false, false>>);
    return launch(a, color_pts_lds_bytes(x3), what, stream);
}

// Projector.compute / compute_view_independent MATERIALISED (models/projector.py:96-425): the four tensors the reference's own
// GeneralRenderingNetwork.forward takes, in its layout.  One wave per (point, view), lane = channel of the 64-float pixel.  Only for callers that
// want the tensors (a foreign rendering network); the fused kernels above never store them.
__global__ __launch_bounds__(256) void k_project_features(ColorMArgs a, float* __restrict__ geo /*[P,16]*/, float* __restrict__ rgb_feat /*[V,P,59]*/,
                                                          float* __restrict__ rdiff /*[V,P,4]*/, float* __restrict__ mask /*[V,P]*/) {
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.n * a.V) return;
    const long long p = w / a.V;
    const int v = (int)(w - p * a.V), c = threadIdx.x & 63;
    const float px = a.pts[3 * p], py = a.pts[3 * p + 1], pz = a.pts[3 * p + 2];
    float gch = 0.f;
    const float msum = trilinear_taps(px, py, pz, a.D, a.maskvol, [&](size_t vox, float wt) {
        if (c < 16) gch = fmaf(a.vol_cl[vox * 16 + c], wt, gch);
    });
    const bool gvalid = point_valid(px, py, pz, msum);
    float qx, qy, qz;
    query_direction(a.normals, a.query_cam, p, px, py, pz, qx, qy, qz);
    const ViewGeom g = view_geom(a, v, px, py, pz, qx, qy, qz, gvalid, 0.f);
    float val = 0.f;
    {
        const Taps2D tp = bilinear_taps(g.gx, g.gy, a.H, a.W_img);
        const float* img = a.cmaps + (size_t)v * a.H * a.W_img * 64 + c;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (tp.w[k] != 0.f) val = fmaf(img[(size_t)tp.idx[k] * 64], tp.w[k], val);
    }
    const size_t vp = (size_t)v * a.n + p;
    if (c < 59) rgb_feat[vp * 59 + c] = val;
    if (c < 4) rdiff[vp * 4 + c] = g.rd[c];
    if (c == 0) mask[vp] = g.m;
    if (v == 0 && c < 16) geo[(size_t)p * 16 + c] = gch;
}

int project_features_launch(const ColorMArgs& a, float* geo, float* rgb_feat, float* rdiff, float* mask, void* stream) {
    hipLaunchKernelGGL(k_project_features, dim3(cdiv(a.n * a.V, 4)), dim3(256), 0, (hipStream_t)stream, a, geo, rgb_feat, rdiff, mask);
    return check_launch("project_features");
}

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
int preload_color_pts() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)(k_project_features));
}
}  // namespace o2345
