// Device helpers shared by the two colour-network kernels (csrc/color_mfma.hip: columns = (point, view) pairs;
// csrc/color_pts.hip: columns = points, views looped): blob layout, matrix-step loops in both numerical forms, the scaled-domain
// ELU, DPP group reductions, projection, and the per-point / per-view stages both evaluate (gather, ray_dir_fc, the per-view network).
// See csrc/color_mfma.hip for the layer structure and weights.pack_color_mfma_blob / pack_color_x3_blob for the operand order.
#pragma once
#include "common.h"
#include "geom_math.h"
#include "split_f16.h"

namespace o2345 {

#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// ---- blob layout (floats) -- must match weights.CM_SEGS / CM_BIAS -------------------------------------------------
constexpr int CM_A_RD0 = 0;                         // [1][2][64]
constexpr int CM_A_RD1 = CM_A_RD0 + 1 * 2 * 64;     // [2][8][64]
constexpr int CM_A_B0 = CM_A_RD1 + 2 * 8 * 64;      // [2][32][64]
constexpr int CM_A_B1 = CM_A_B0 + 2 * 32 * 64;      // [1][32][64]
constexpr int CM_A_V0 = CM_A_B1 + 32 * 64;          // [1][16][64]
constexpr int CM_A_V1 = CM_A_V0 + 16 * 64;          // [1][16][64]  (rows 0..31 of vis_fc.2; row 32 is a dot product)
constexpr int CM_A_V20 = CM_A_V1 + 16 * 64;         // [1][16][64]
constexpr int CM_A_R0 = CM_A_V20 + 16 * 64;         // [1][19][64]
constexpr int CM_A_R1 = CM_A_R0 + 19 * 64;          // [1][8][64]
constexpr int CM_BIAS0 = CM_A_R1 + 8 * 64;          // biases / per-lane vectors, [block][half][16] each
constexpr int CM_B_RD0 = CM_BIAS0, CM_B_RD1 = CM_B_RD0 + 32, CM_B_B0 = CM_B_RD1 + 64, CM_B_B1 = CM_B_B0 + 64,
              CM_B_V0 = CM_B_B1 + 32, CM_B_V1 = CM_B_V0 + 32, CM_B_V20 = CM_B_V1 + 32, CM_B_R0 = CM_B_V20 + 32,
              CM_B_R1 = CM_B_R0 + 32, CM_V_V1X = CM_B_R1 + 32, CM_V_V21 = CM_V_V1X + 32, CM_V_R2 = CM_V_V21 + 32;
constexpr int CM_W_S = CM_V_R2 + 32;                // [144][64]
constexpr int CM_S = CM_W_S + 144 * 64;             // [s, bias vis_fc.2[32], bias vis_fc2.2, bias rgb_fc.4]
constexpr int CM_TOTAL = CM_S + 4;
// split-f16 blob: A segments [block][k-step of 16][hi|lo][64 lanes][8 f16 = 4 floats], then the fp32 tail (CM_BIAS0 .. CM_TOTAL)
constexpr int CX_A_RD0 = 0;                         // [1][1]
constexpr int CX_A_RD1 = CX_A_RD0 + 1 * 1 * 512;    // [2][1]
constexpr int CX_A_B0 = CX_A_RD1 + 2 * 1 * 512;     // [2][4]
constexpr int CX_A_B1 = CX_A_B0 + 2 * 4 * 512;      // [1][4]
constexpr int CX_A_V0 = CX_A_B1 + 4 * 512;          // [1][2]
constexpr int CX_A_V1 = CX_A_V0 + 2 * 512;          // [1][2]
constexpr int CX_A_V20 = CX_A_V1 + 2 * 512;         // [1][2]
constexpr int CX_A_R0 = CX_A_V20 + 2 * 512;         // [1][3]
constexpr int CX_A_R1 = CX_A_R0 + 3 * 512;          // [1][1]
constexpr int CX_A_END = CX_A_R1 + 1 * 512;
constexpr int CX_TOTAL = CX_A_END + (CM_TOTAL - CM_BIAS0);
// The view-independent rows of base_fc.0 (geo | mean | var -> 64) once more as a matrix-core A operand, for csrc/color_pts.hip where a
// column is a POINT and the rows are evaluated by MFMA (2 output blocks, 72 per-half operands: 8 geometry channels, 32 means, 32
// variances of the half's pixel floats).  Appended behind the tail so that the prefix read by k_color_mfma is unchanged.
constexpr int CM_A_S = CM_TOTAL;                    // fp32 form [2][72][64]
constexpr int CM_TOTAL2 = CM_A_S + 2 * 72 * 64;
constexpr int CX_A_S = CX_TOTAL;                    // split-f16 form [2][9 k-steps][hi|lo][64][8 f16]
constexpr int CX_TOTAL2 = CX_A_S + 2 * 9 * 512;

struct ColorMArgs {
    const float* blob;
    const float* vol_cl; const float* maskvol; int D;
    const float* cmaps; const float* proj; const float* cam_pos; int V, H, W_img;
    const float* pts; const int* index; const int* n_dev; long long n;
    const float* query_cam; const float* normals;
    float* out_rgb; uint8_t* out_nviews;
    // materialised inputs of GeneralRenderingNetwork.forward (k_color_pts<.., FEATS = true> only): the reference's view-major tensors
    const float* f_geo;       // [P,16]
    const float* f_rgb;       // [V,P,59]  colours (3) | features (56)
    const float* f_rdiff;     // [V,P,4]
    const float* f_mask;      // [V,P]     non-zero = the projection is valid
    unsigned long long* stats;  // optional caller-owned device counters (stats_dev of o2345_color_points_*): [0] += (tile, view) pairs evaluated in pass A, [1] += in pass B,
                              // [2] += tiles, [3] += tiles that evaluated every view in pass B because one of their points has no visible view
    int sched;                // scheduling knobs (O2345_COLOR_SCHED; default 10 = bits 1 + 3, measured on MI355X, profiles/NOTES.md "Wave priorities in the colour kernels"):
                              //   bit 0  static wave priority by SIMD slot (the k-th wave of a SIMD runs at priority k): no gain
                              //   bit 1  priority 3 while a wave issues its pixel gathers: -1.5 %
                              //   bit 2  k_color_pts evaluates EVERY view (no skipping of views that see none of a tile's points): +13 % (the round-2 kernel)
                              //   bit 3  k_color_pts: block-interleaved tile schedule instead of one contiguous eighth of the list per XCD -- with view
                              //          skipping a tile's cost depends on where its rays look: -1 % at 8 views, -20 % at 32 views (the statically dealt
                              //          tiles only: with a tile queue, below, the render call deals none)
                              //   bit 4  k_color_pts evaluates zero-weight pooling views (no skipping, in pass A, of a view that every point of the tile
                              //          sees with pooling weight 0; bit 2 turns this skipping off as well)
    int* tile_queue;          // optional tile queue of k_color_pts (common.h: TQ_HEADS ints, zero at launch): the tail of the tile list is claimed by the waves
                              // that have finished their static share.  Null: the static schedule alone.
};

inline int color_sched_mode() { return knobs().color_sched; }
#if defined(__HIPCC__)
__device__ __forceinline__ void set_wave_prio(int p) {       // s_setprio takes an immediate
    switch (p) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
    }
}
#endif

// ELU is evaluated ~150 times per lane and tile (a quarter of the kernel's VALU instructions), so the whole network runs in a
// log2(e)-scaled domain: every layer that feeds an ELU produces y = log2(e) * x (its weights / bias are pre-scaled on the host,
// weights.pack_color_mfma_blob) and the activation is   ELU_y(y) = log2(e) * ELU(x) = max(y, log2(e) * (min(2^y, 1) - 1)):
// v_exp_f32 with its [0,1] output clamp, one fma, one max -- no multiply by log2(e) in front of the exponential.  The scale
// cancels in the next layer (ln2 * log2e = 1, so hidden-layer weights are unchanged; only biases and the first / last layers
// carry a factor).  e^x - 1 has an ABSOLUTE error of ~1e-7 (one ulp of 1.0), which is what matters downstream.
// Reciprocals are the hardware v_rcp_f32 (1 ulp) instead of the ~10-instruction IEEE division sequence.
constexpr float LOG2E = 1.44269504088896340736f, LN2 = 0.69314718055994530942f;
__device__ __forceinline__ float celu(float y) {
    const float t = __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(y), 0.f, 1.f);
    return fmaxf(y, fmaf(t, LOG2E, -LOG2E));
}
// two at a time: the multiply-add is one packed-fp32 instruction for both (consecutive accumulator registers are an aligned pair)
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 celu2(float y0, float y1) {
    f32x2 t;
    t[0] = __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(y0), 0.f, 1.f);
    t[1] = __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(y1), 0.f, 1.f);
    const f32x2 e = __builtin_elementwise_fma(t, f32x2{LOG2E, LOG2E}, f32x2{-LOG2E, -LOG2E});
    return f32x2{fmaxf(y0, e[0]), fmaxf(y1, e[1])};
}
__device__ __forceinline__ float crcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float csigm(float z) { return crcp(1.f + __builtin_amdgcn_exp2f(-z)); }      // sigmoid of z / log2(e)

// NB output blocks, N k-steps whose B operands are b[0..N-1]; A operands come from LDS, next step prefetched
template <int NB, int NST, int N>
__device__ __forceinline__ void cm_run(f32x16 (&acc)[NB], const float* A /* + lane */, int step0, const float (&b)[N]) {
    float cur[NB], nxt[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) cur[nb] = A[(nb * NST + step0) * 64];
#pragma unroll
    for (int r = 0; r < N; ++r) {
        if (r + 1 < N) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) nxt[nb] = A[(nb * NST + step0 + r + 1) * 64];
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = MFMA32(cur[nb], b[r], acc[nb]);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) cur[nb] = nxt[nb];
        __builtin_amdgcn_sched_barrier(0);
    }
}

// split-f16 form of the same step loop (csrc/split_f16.h): b[] is the per-half operand list of the fp32 form, consumed 8 per MFMA step.  lo in the
// C form: the asm form measured 40.9 vs 39.6 ms for k_color_pts (the two-instruction asm block constrains the scheduler more than it saves).
// The three MFMA loops are written out here: routed through mfma_x3 they come out with a different register assignment in k_color_pts.
template <int NB, int N>
__device__ __forceinline__ void cx_run(f32x16 (&acc)[NB], const float4* A /* segment + lane */, const float (&b)[N], float m1) {
    constexpr int NS = (N + 7) / 8;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const Split8 sp = split8(b, 8 * s, m1);
        h16x8 ahi[NB], alo[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            ahi[nb] = __builtin_bit_cast(h16x8, A[((nb * NS + s) * 2 + 0) * 64]);
            alo[nb] = __builtin_bit_cast(h16x8, A[((nb * NS + s) * 2 + 1) * 64]);
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = MFMA_F16(alo[nb], sp.hi, acc[nb]);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = MFMA_F16(ahi[nb], sp.lo, acc[nb]);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = MFMA_F16(ahi[nb], sp.hi, acc[nb]);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// one layer's matrix part in either form
template <bool X3, int NB, int N>
__device__ __forceinline__ void cm_layer(f32x16 (&acc)[NB], const float* lds, int lane, int off32, int offx, const float (&b)[N], float m1) {
    if constexpr (X3) cx_run<NB, N>(acc, reinterpret_cast<const float4*>(lds + offx) + lane, b, m1);
    else cm_run<NB, N, N>(acc, lds + lane + off32, 0, b);
}

// biases are stored [block][half][16 registers]: four 16-byte LDS reads straight into the accumulator tuple
template <int NB>
__device__ __forceinline__ void cm_bias(f32x16 (&acc)[NB], const float* bias, int h) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const float4* p = reinterpret_cast<const float4*>(bias + (nb * 2 + h) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 t = p[q];
            acc[nb][4 * q] = t.x; acc[nb][4 * q + 1] = t.y; acc[nb][4 * q + 2] = t.z; acc[nb][4 * q + 3] = t.w;
        }
    }
}

// Reductions over the G view lanes of a point (G consecutive lanes, G | 32) with DPP lane permutes instead of
// ds_bpermute: xor 1 / xor 2 are quad_perm, then row_half_mirror (i <-> 7-i) and row_mirror (i <-> 15-i) combine quads
// that already hold their own partial result; only the 16 <-> 16 step of G = 32 goes through the LDS crossbar.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
#define O2345_GROUP_REDUCE(NAME, OP)                                                   \
    template <int G>                                                                   \
    __device__ __forceinline__ float NAME(float v) {                                   \
        v = OP(v, dpp_mov<0xB1>(v));                        /* quad_perm [1,0,3,2] */  \
        v = OP(v, dpp_mov<0x4E>(v));                        /* quad_perm [2,3,0,1] */  \
        if (G >= 8) v = OP(v, dpp_mov<0x141>(v));           /* row_half_mirror     */  \
        if (G >= 16) v = OP(v, dpp_mov<0x140>(v));          /* row_mirror          */  \
        if (G >= 32) v = OP(v, __shfl_xor(v, 16));                                     \
        return v;                                                                      \
    }
__device__ __forceinline__ float op_add(float a, float b) { return a + b; }
O2345_GROUP_REDUCE(gsum, op_add)
O2345_GROUP_REDUCE(gmin, fminf)
O2345_GROUP_REDUCE(gmax, fmaxf)
#undef O2345_GROUP_REDUCE

__device__ __forceinline__ void cm_project(const float* __restrict__ P, float x, float y, float z, int H, int W, float& gx, float& gy) {
    const float X = project_row(P, x, y, z);
    const float Y = project_row(P + 4, x, y, z);
    const float Z = fmaxf(project_row(P + 8, x, y, z), 1e-3f);
    // a / b as a * rcp(b) with one Newton step on the quotient (q += (a - b q) * r): within 1 ulp of the IEEE quotient (almost
    // always identical) in 3 instructions instead of the ~12 of the division sequence; the reciprocals are shared
    const float rz = crcp(Z), rw = crcp((float)(W - 1)), rh = crcp((float)(H - 1));
    auto div = [](float a_, float b_, float r_) { const float q = a_ * r_; return fmaf(fmaf(-b_, q, a_), r_, q); };
    gx = div(2.f * div(X, Z, rz), (float)(W - 1), rw) - 1.f;
    gy = div(2.f * div(Y, Z, rz), (float)(H - 1), rh) - 1.f;
    if (gx > 1.f || gx < -1.f) gx = 2.f;
    if (gy > 1.f || gy < -1.f) gy = 2.f;
}


#if defined(__HIPCC__)
// Per-point and per-view stages that every colour kernel evaluates the same way (k_color_pts and k_project_features of csrc/color_pts.hip, the
// test-only k_color_mfma of csrc/color_mfma.hip).  What differs between the kernels -- work decomposition, reductions over the views, the LDS exchange of
// the shared rows -- stays with them.

// d[4q .. 4q+3] += w * p4[q] for Q consecutive 16-byte loads (the taps of the geometry feature)
template <int Q>
__device__ __forceinline__ void fma_rows(const float4* p4, float w, float* d) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const float4 t = p4[q];
        d[4 * q] = fmaf(t.x, w, d[4 * q]); d[4 * q + 1] = fmaf(t.y, w, d[4 * q + 1]);
        d[4 * q + 2] = fmaf(t.z, w, d[4 * q + 2]); d[4 * q + 3] = fmaf(t.w, w, d[4 * q + 3]);
    }
}

// The non-zero ones of the 8 trilinear taps of point p in the D^3 volumes: f(voxel index, weight) for each, in tap order; returns the mask sum.
template <class F>
__device__ __forceinline__ float trilinear_taps(float px, float py, float pz, int D, const float* __restrict__ maskvol, F&& f) {
    const Axis2 ax = axis_taps_zeros(px, D), ay = axis_taps_zeros(py, D), az = axis_taps_zeros(pz, D);
    float msum = 0.f;
#pragma unroll
    for (int tap = 0; tap < 8; ++tap) {
        const int ia = (tap >> 2) & 1, ib = (tap >> 1) & 1, ic = tap & 1;
        const float w = ax.w[ia] * ay.w[ib] * az.w[ic];
        if (w != 0.f) {
            const size_t vox = ((size_t)ax.i[ia] * D + ay.i[ib]) * D + az.i[ic];
            msum += w * maskvol[vox];
            f(vox, w);
        }
    }
    return msum;
}
// the geometry feature of a point counts if the point lies inside the volume and its taps' mask sum is positive
__device__ __forceinline__ bool point_valid(float px, float py, float pz, float msum) {
    return fabsf(px) < 1.f && fabsf(py) < 1.f && fabsf(pz) < 1.f && msum > 0.f;
}

// direction the point is looked at from: its normalised normal (compute_view_independent) or the normalised query_cam - p (Projector.compute)
__device__ __forceinline__ void query_direction(const float* __restrict__ normals, const float* __restrict__ query_cam, long long slot, float px, float py,
                                                float pz, float& qx, float& qy, float& qz) {
    if (normals) {
        const float nx = normals[3 * slot], ny = normals[3 * slot + 1], nz = normals[3 * slot + 2];
        const float rn = crcp(fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), 1e-6f));
        qx = nx * rn; qy = ny * rn; qz = nz * rn;
    } else {
        const float tx = query_cam[0] - px, ty = query_cam[1] - py, tz = query_cam[2] - pz;
        const float rn = crcp(sqrtf(tx * tx + ty * ty + tz * tz) + 1e-6f);
        qx = tx * rn; qy = ty * rn; qz = tz * rn;
    }
}

// geometry of one source view for this lane's point: ray_diff (4), pooling exponent, projection mask and the bilinear taps
struct ViewGeom {
    float rd[4];
    float e;          // 2^(s_abs * (dot - 1))
    float m;          // 1 if the point is valid and projects inside view v
    float gx, gy;
};

__device__ __forceinline__ ViewGeom view_geom(const ColorMArgs& a, int v, float px, float py, float pz, float qx, float qy, float qz,
                                              bool gvalid, float s_abs) {
    ViewGeom g;
    cm_project(a.proj + 12 * v, px, py, pz, a.H, a.W_img, g.gx, g.gy);
    g.m = (gvalid && fabsf(g.gx) < 1.f && fabsf(g.gy) < 1.f) ? 1.f : 0.f;
    const float sx = a.cam_pos[3 * v] - px, sy = a.cam_pos[3 * v + 1] - py, sz = a.cam_pos[3 * v + 2] - pz;
    const float rsn = crcp(sqrtf(sx * sx + sy * sy + sz * sz) + 1e-6f);
    const float ux = sx * rsn, uy = sy * rsn, uz = sz * rsn;
    const float dx = qx - ux, dy = qy - uy, dz = qz - uz;
    const float rdn = crcp(fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-6f));
    g.rd[0] = dx * rdn; g.rd[1] = dy * rdn; g.rd[2] = dz * rdn;
    g.rd[3] = qx * ux + qy * uy + qz * uz;
    g.e = __builtin_amdgcn_exp2f(s_abs * (g.rd[3] - 1.f));       // s_abs carries log2(e)
    return g;
}

// this half's 32 pixel floats of view v at (g.gx, g.gy), bilinear, ATen zero padding, in the log2(e)-scaled domain.
// (Measured alternatives in k_color_pts, all slower on MI355X: branch-free taps 50-59 ms; taps of view v + 1 requested during the network of view v
// -- one tap, 32 registers, at a time -- 48.4 ms; lane octets fetching whole 128-byte half pixels through global_load_lds into a per-wave
// LDS staging area (8 lines per instruction instead of up to 64) 48.9 ms; this form 44.5-45.2 ms.  See DESIGN.md section 8.)
// The tap is written out: through fma_rows<8> k_color_pts accumulates in place and moves 112 registers more per gather.
__device__ __forceinline__ void gather_now(const ColorMArgs& a, int h, int v, const ViewGeom& g, float (&rf)[32]) {
#pragma unroll
    for (int c = 0; c < 32; ++c) rf[c] = 0.f;
    const Taps2D tp = bilinear_taps(g.gx, g.gy, a.H, a.W_img);
    const float4* img = reinterpret_cast<const float4*>(a.cmaps + (size_t)v * a.H * a.W_img * 64) + 8 * h;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (tp.w[k] != 0.f) {
            const float4* px4 = img + (size_t)tp.idx[k] * 16;
            const float wk = tp.w[k] * LOG2E;                       // pixel floats enter the network in the scaled domain
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 t = px4[q];
                rf[4 * q] = fmaf(t.x, wk, rf[4 * q]); rf[4 * q + 1] = fmaf(t.y, wk, rf[4 * q + 1]);
                rf[4 * q + 2] = fmaf(t.z, wk, rf[4 * q + 2]); rf[4 * q + 3] = fmaf(t.w, wk, rf[4 * q + 3]);
            }
        }
}

// ray_dir_fc (4 -> 16 -> 59) of ray difference rd, added to this half's 32 gathered pixel floats.  `tail`: shift of the bias block in the staged blob
// (X3 ? CX_A_END - CM_BIAS0 : 0), here and below.
template <bool X3>
__device__ __forceinline__ void add_direction_feature(const float* lds, int tail, int lane, int h, const float (&rd)[4], float m1, float (&rf)[32]) {
    f32x16 acc1[1];
    cm_bias<1>(acc1, lds + tail + CM_B_RD0, h);
    const float b0[2] = {h ? rd[1] : rd[0], h ? rd[3] : rd[2]};
    cm_layer<X3, 1, 2>(acc1, lds, lane, CM_A_RD0, CX_A_RD0, b0, m1);
    float d16[8];
#pragma unroll
    for (int r = 0; r < 8; r += 2) { const f32x2 e2 = celu2(acc1[0][r], acc1[0][r + 1]); d16[r] = e2[0]; d16[r + 1] = e2[1]; }
    f32x16 acc2[2];
    cm_bias<2>(acc2, lds + tail + CM_B_RD1, h);
    cm_layer<X3, 2, 8>(acc2, lds, lane, CM_A_RD1, CX_A_RD1, d16, m1);
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; r += 2) { const f32x2 e2 = celu2(acc2[b][r], acc2[b][r + 1]); rf[16 * b + r] += e2[0]; rf[16 * b + r + 1] += e2[1]; }
}

// The network of one (point, view) pair behind the view-independent rows: base_fc -> vis_fc -> vis_fc2 -> rgb_fc, returns the pair's blending score
// (scaled domain).  acc: the starting accumulator of base_fc.0, i.e. bias + view-independent rows (geo | mean | var) of the point; rf: this half's
// pixel floats + direction feature; wgt: normalised pooling weight; m: the view's mask; sc: the four scalars of the blob (CM_S).
template <bool X3>
__device__ __forceinline__ float view_network(f32x16 (&acc)[2], const float (&rf)[32], const float (&rd)[4], float wgt, float m, float m1,
                                              const float* lds, int tail, const float* sc, int lane, int h) {
    // ---- base_fc: (shared + 59 per-view features) -> 64 -> 32
    f32x16 x32[1];
    {
        cm_layer<X3, 2, 32>(acc, lds, lane, CM_A_B0, CX_A_B0, rf, m1);
        float hb[32];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; r += 2) { const f32x2 e2 = celu2(acc[b][r], acc[b][r + 1]); hb[16 * b + r] = e2[0]; hb[16 * b + r + 1] = e2[1]; }
        cm_bias<1>(x32, lds + tail + CM_B_B1, h);
        cm_layer<X3, 1, 32>(x32, lds, lane, CM_A_B1, CX_A_B1, hb, m1);
#pragma unroll
        for (int r = 0; r < 16; r += 2) { const f32x2 e2 = celu2(x32[0][r], x32[0][r + 1]); x32[0][r] = e2[0]; x32[0][r + 1] = e2[1]; }
    }
    // ---- vis_fc
    float vis;
    {
        float bin[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) bin[r] = x32[0][r] * wgt;
        f32x16 t1[1];
        cm_bias<1>(t1, lds + tail + CM_B_V0, h);
        cm_layer<X3, 1, 16>(t1, lds, lane, CM_A_V0, CX_A_V0, bin, m1);
#pragma unroll
        for (int r = 0; r < 16; r += 2) { const f32x2 e2 = celu2(t1[0][r], t1[0][r + 1]); bin[r] = e2[0]; bin[r + 1] = e2[1]; }
        f32x16 t2[1];
        cm_bias<1>(t2, lds + tail + CM_B_V1, h);
        cm_layer<X3, 1, 16>(t2, lds, lane, CM_A_V1, CX_A_V1, bin, m1);
        float vr = 0.f;                                           // output 32 of vis_fc.2: dot product over both halves
#pragma unroll
        for (int r = 0; r < 16; ++r) vr = fmaf(bin[r], lds[tail + CM_V_V1X + h * 16 + r], vr);
        vr += __shfl_xor(vr, 32);
#pragma unroll
        for (int r = 0; r < 16; r += 2) { const f32x2 e2 = celu2(t2[0][r], t2[0][r + 1]); x32[0][r] += e2[0]; x32[0][r + 1] += e2[1]; }
        vis = csigm(celu(vr + sc[1])) * m;
    }
    // ---- vis_fc2
    {
        float bin[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) bin[r] = x32[0][r] * vis;
        f32x16 t1[1];
        cm_bias<1>(t1, lds + tail + CM_B_V20, h);
        cm_layer<X3, 1, 16>(t1, lds, lane, CM_A_V20, CX_A_V20, bin, m1);
#pragma unroll
        for (int r = 0; r < 16; r += 2) { const f32x2 e2 = celu2(t1[0][r], t1[0][r + 1]); bin[r] = e2[0]; bin[r + 1] = e2[1]; }
        float vr = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) vr = fmaf(bin[r], lds[tail + CM_V_V21 + h * 16 + r], vr);
        vr += __shfl_xor(vr, 32);
        vis = csigm(vr + sc[2]) * m;
    }
    // ---- rgb_fc: [x | vis | ray_diff] (37) -> 16 -> 8 -> 1
    float bin[19];
#pragma unroll
    for (int r = 0; r < 16; ++r) bin[r] = x32[0][r];
    bin[16] = h ? rd[0] : vis; bin[17] = h ? rd[2] : rd[1]; bin[18] = h ? 0.f : rd[3];
    f32x16 t1[1];
    cm_bias<1>(t1, lds + tail + CM_B_R0, h);
    cm_layer<X3, 1, 19>(t1, lds, lane, CM_A_R0, CX_A_R0, bin, m1);
    float r16[8];
#pragma unroll
    for (int r = 0; r < 8; r += 2) { const f32x2 e2 = celu2(t1[0][r], t1[0][r + 1]); r16[r] = e2[0]; r16[r + 1] = e2[1]; }
    f32x16 t2[1];
    cm_bias<1>(t2, lds + tail + CM_B_R1, h);
    cm_layer<X3, 1, 8>(t2, lds, lane, CM_A_R1, CX_A_R1, r16, m1);
    float r8[4];
#pragma unroll
    for (int r = 0; r < 4; r += 2) { const f32x2 e2 = celu2(t2[0][r], t2[0][r + 1]); r8[r] = e2[0]; r8[r + 1] = e2[1]; }
    float sr = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) sr = fmaf(r8[r], lds[tail + CM_V_R2 + h * 16 + r], sr);
    return sr + __shfl_xor(sr, 32) + sc[3];
}
#endif

// csrc/color_pts.hip (the product kernels; csrc/color_mfma.hip holds the entry points, which check their arguments and fill the ColorMArgs).
// k_color_pts<x3, feats> on a: feats = the materialised inputs f_* instead of the point's own projection
int color_pts_launch(const ColorMArgs& a, int x3, bool feats, const char* what, void* stream);
int project_features_launch(const ColorMArgs& a, float* geo, float* rgb_feat, float* rdiff, float* mask, void* stream);

}  // namespace o2345
