// Shared pieces of the SDF-network kernels (csrc/sdf_mlp.hip: exact fp32 MFMA; csrc/sdf_mlp_x3.hip: split-f16 operands): blob geometry, LDS layouts, argument block, softplus, the per-point stages every kernel runs (point of the tile lane, latent gather, positional encoding, bias, softplus + split, chain rule, latent Jacobian), A-operand fetch, the pinned MFMA step loop and the launch body.
#pragma once
#include "common.h"
#include "geom_math.h"
#include "pe_math.h"
#include "split_f16.h"

namespace o2345 {

// ---- blob geometry (must match one-2-3-45_amd/weights.py) --------------------------------------------------------
constexpr int ST0 = 20;          // layer-0 k steps  (40 PE slots = 39 + 1 pad)
constexpr int ST1 = 72;          // layer-1/2 k steps (64 hidden + 8 latent)
constexpr int STB = 64;          // backward k steps (128 upstream neurons)
constexpr int OFF_A0 = 0;                          // [4][ST0][64]
constexpr int OFF_A1 = OFF_A0 + 4 * ST0 * 64;      // [4][ST1][64]
constexpr int OFF_A2 = OFF_A1 + 4 * ST1 * 64;      // [4][ST1][64]
constexpr int OFF_A1T = OFF_A2 + 4 * ST1 * 64;     // [5][STB][64]   d/d(h0 | latent)
constexpr int OFF_A0T = OFF_A1T + 5 * STB * 64;    // [2][STB][64]   d/d(pe)
constexpr int OFF_MISC = OFF_A0T + 2 * STB * 64;   // b0[128] b1[128] b2[128] w2row_h[128] w2row_lat[16] (lane-half order)
constexpr int MISC_B0 = 0, MISC_B1 = 128, MISC_B2 = 256, MISC_W2H = 384, MISC_W2L = 512, MISC_SIZE = 528;
constexpr int BLOB_F32_FLOATS = OFF_MISC + MISC_SIZE;
constexpr int OFFX_MISC = BLOB_F32_FLOATS;         // the split-f16 kernels' MISC block: b0, b1 in the t domain (weights.py SOFTPLUS_SCALE), the rest as above
// split-f16 ("f16x3") copies for csrc/sdf_mlp_x3.hip: every weight as hi = f16(w), lo = f16(w - hi);
// [block][k-step of 16][hi|lo][64 lanes][8 f16 = 4 floats]
constexpr int STX0 = 3;                                  // layer-0 k steps of 16 (2 x 20 PE slots padded to 2 x 24)
constexpr int STH1 = 9;                                  // layer-1 k steps of 16 (8 hidden + 1 latent)
constexpr int STHB = 8;                                  // backward k steps of 16 (128 upstream neurons)
constexpr int OFFX_A0 = OFFX_MISC + MISC_SIZE;           // [4][STX0][2][64][4]
static_assert(OFFX_A0 % 4 == 0, "the float4 staging and the b128 buffer loads of the split-f16 sections need 16-byte alignment");
constexpr int OFFX_A1 = OFFX_A0 + 4 * STX0 * 2 * 256;    // [4][STH1][2][64][4]
constexpr int OFFX_A1T = OFFX_A1 + 4 * STH1 * 2 * 256;   // [5][STHB][2][64][4]
constexpr int OFFX_A0T = OFFX_A1T + 5 * STHB * 2 * 256;  // [2][STHB][2][64][4]
constexpr int BLOB_FLOATS = OFFX_A0T + 2 * STHB * 2 * 256;

enum : int { VAR_SDF = 0, VAR_FULL = 1, VAR_GRAD = 2 };

// ---- LDS layouts in floats, all dynamic: the kernels index with them and the launchers size the allocation from them ------------------------------
// k_sdf_mlp<VARIANT>:  VAR_SDF : A0 | A1 | misc           VAR_FULL : A1 | A2 | misc          VAR_GRAD : A1 | A1T | misc
constexpr int N_A0 = 4 * ST0 * 64, N_A1 = 4 * ST1 * 64, N_A1T = 5 * STB * 64;
constexpr int sdf_lds_first(int variant) { return variant == VAR_SDF ? N_A0 : N_A1; }
constexpr int sdf_lds_second(int variant) { return variant == VAR_GRAD ? N_A1T : N_A1; }
constexpr int sdf_lds_floats(int variant) { return sdf_lds_first(variant) + sdf_lds_second(variant) + MISC_SIZE; }
// k_sdf_mlp_x3: A0 | A1 | misc;  k_sdf_grad_x3: A0 | A1 | output blocks 0-2 of A1T | misc  (the sections are adjacent in the blob, in this order)
constexpr int NX_A0 = 4 * STX0 * 2 * 256, NX_A1 = 4 * STH1 * 2 * 256, NX_A1T3 = 3 * STHB * 2 * 256;
constexpr int LDSX_MLP_FLOATS = NX_A0 + NX_A1 + MISC_SIZE;
constexpr int LDSX_GRAD_FLOATS = NX_A0 + NX_A1 + NX_A1T3 + MISC_SIZE;

struct SdfArgs {
    const float* blob;        // BLOB_FLOATS floats
    const float* vol_cl;      // [D,D,D,16] channel-last latent volume
    int D;
    const float* pts;         // [P,3] (mode 0) or null (mode 1: x-major grid of side R on linspace(-1,1,R))
    const int* index;         // optional gather/scatter list: point i is pts[index[i]] and results go to slot index[i]
    const int* n_dev;         // optional device-side count overriding n
    long long n;
    int R;
    float sign;               // sdf output multiplier (extract_fields stores u = -sdf)
    float* out_sdf;           // [P]
    float* out_feat;          // [P,128] or null (VAR_FULL)
    float* out_lat;           // [P,16] or null
    float* out_grad;          // [P,3] or null (VAR_GRAD)
    const float* lat_in;      // optional [P,16]: use this latent instead of sampling the volume (get_sdf_volume)
    // lattice mode of k_sdf_mlp_x3 only: layer 0 tabulated per axis (weights.sdf_grid_tables): its pre-activation is separable on the lattice,
    // a0(ix,iy,iz) = b0 + Tx[ix] + Ty[iy] + Tz[iz]; rows of 128 floats in lane order [wave half][accumulator block * 16 + register]
    const float* tab_xy;      // [R*R][128] = b0 + Tx[ix] + Ty[iy]
    const float* tab_z;       // [R][128]
};

// Softplus(beta=100, threshold=20) and its derivative (torch: x if 100x > 20 else log1p(exp(100x))/100; backward
// z/(z+1)).  The network evaluates 256 of these per point and the kernels are VALU-bound, so this is written for the
// hardware exp2/log2 units:  softplus(a) = max(a,0) + log1p(e)/100,  e = exp(-|100a|) in (0,1].
// log1p(e) is taken as ln2*log2(fl(1+e)): the rounding of 1+e is an ABSOLUTE error of <= 6e-8 in the logarithm, i.e.
// <= 6e-10 in the result after the /100 -- far below the fp32 resolution of the O(0.1) pre-activations it is added to
// (a relative-accuracy correction of the tiny tail would cost 6 more instructions per call and buys nothing).
// For 100a > 16.7, fl(1+e) == 1 and the result is exactly a, which also realises torch's threshold branch.
__device__ __forceinline__ float softplus100(float a, float& dsig) {
    const float e = __builtin_amdgcn_exp2f(fabsf(a) * -144.269504088896340736f);     // exp(-|100 a|)
    const float u = 1.f + e;
    const float l2 = __builtin_amdgcn_logf(u);                                       // log2(1 + e)
    dsig = (a >= 0.f ? 1.f : e) * __builtin_amdgcn_rcpf(u);                           // sigmoid(100 a); dead code unless used
    return fmaf(l2, 0.00693147180559945309f, fmaxf(a, 0.f));
}

// Two at a time: the multiply, the 1 + e and the final multiply-add are packed fp32 instructions (v_pk_mul/add/fma_f32 work
// on an even-aligned register pair -- consecutive accumulator registers are one), -|t| rides on v_exp_f32's source modifiers:
// 4.5 instructions per value instead of 6.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 softplus100_pair(f32x2 a) {
    const f32x2 t = a * 144.269504088896340736f;
    f32x2 e;
    e[0] = __builtin_amdgcn_exp2f(-__builtin_fabsf(t[0]));
    e[1] = __builtin_amdgcn_exp2f(-__builtin_fabsf(t[1]));
    const f32x2 u = e + 1.f;
    f32x2 l, m;
    l[0] = __builtin_amdgcn_logf(u[0]); l[1] = __builtin_amdgcn_logf(u[1]);
    m[0] = fmaxf(a[0], 0.f); m[1] = fmaxf(a[1], 0.f);
    return __builtin_elementwise_fma(l, f32x2{0.00693147180559945309f, 0.00693147180559945309f}, m);
}

// value and derivative for a pair: sigmoid(100 a) = 1/u for a >= 0 and 1 - 1/u for a < 0, i.e. 0.5 + copysign(1/u - 0.5, a)
__device__ __forceinline__ f32x2 softplus100_pair(f32x2 a, f32x2& dsig) {
    const f32x2 t = a * 144.269504088896340736f;
    f32x2 e;
    e[0] = __builtin_amdgcn_exp2f(-__builtin_fabsf(t[0]));
    e[1] = __builtin_amdgcn_exp2f(-__builtin_fabsf(t[1]));
    const f32x2 u = e + 1.f;
    f32x2 l, m, ru;
    l[0] = __builtin_amdgcn_logf(u[0]); l[1] = __builtin_amdgcn_logf(u[1]);
    ru[0] = __builtin_amdgcn_rcpf(u[0]); ru[1] = __builtin_amdgcn_rcpf(u[1]);
    m[0] = fmaxf(a[0], 0.f); m[1] = fmaxf(a[1], 0.f);
    f32x2 q = ru - 0.5f;
    q[0] = __builtin_copysignf(q[0], a[0]); q[1] = __builtin_copysignf(q[1], a[1]);
    dsig = q + 0.5f;
    return __builtin_elementwise_fma(l, f32x2{0.00693147180559945309f, 0.00693147180559945309f}, m);
}

// ---- the same in the t domain (csrc/sdf_mlp_x3.hip): t = 100 a / ln 2 arrives from the matrix cores (the factor is folded into the packed operands,
// weights.py SOFTPLUS_SCALE) and the activation leaves as s' = softplus(a) * 100 / ln 2 = max(t, 0) + log2(1 + 2^-|t|): no multiply in front, a plain add
// at the end -- 5 vector instructions per value instead of 6.  For t > 24, fl(1 + 2^-t) == 1 and s' == t exactly (torch's threshold branch, 100 a > 20
// <=> t > 28.9).  softplus'(a) = sigmoid(100 a) = sigmoid(t ln 2) = 1 / (1 + 2^-t).
constexpr float SOFTPLUS_INV_SCALE = 0.00693147180559945309f;                           // ln 2 / 100: applied ONCE per point, to the SDF row's hidden sum
__device__ __forceinline__ f32x2 softplus_t_pair(f32x2 t) {
    f32x2 e;
    e[0] = __builtin_amdgcn_exp2f(-__builtin_fabsf(t[0]));
    e[1] = __builtin_amdgcn_exp2f(-__builtin_fabsf(t[1]));
    const f32x2 u = e + 1.f;
    f32x2 l, m;
    l[0] = __builtin_amdgcn_logf(u[0]); l[1] = __builtin_amdgcn_logf(u[1]);
    m[0] = fmaxf(t[0], 0.f); m[1] = fmaxf(t[1], 0.f);
    return l + m;
}
__device__ __forceinline__ f32x2 softplus_t_pair(f32x2 t, f32x2& dsig) {
    f32x2 e;
    e[0] = __builtin_amdgcn_exp2f(-__builtin_fabsf(t[0]));
    e[1] = __builtin_amdgcn_exp2f(-__builtin_fabsf(t[1]));
    const f32x2 u = e + 1.f;
    f32x2 l, m, ru;
    l[0] = __builtin_amdgcn_logf(u[0]); l[1] = __builtin_amdgcn_logf(u[1]);
    ru[0] = __builtin_amdgcn_rcpf(u[0]); ru[1] = __builtin_amdgcn_rcpf(u[1]);
    m[0] = fmaxf(t[0], 0.f); m[1] = fmaxf(t[1], 0.f);
    f32x2 q = ru - 0.5f;
    q[0] = __builtin_copysignf(q[0], t[0]); q[1] = __builtin_copysignf(q[1], t[1]);
    dsig = q + 0.5f;
    return l + m;
}
__device__ __forceinline__ float softplus_t_d(float t) {
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-t));
}

// derivative only (the gradient kernels re-evaluate layer 0 just for this): sigmoid(100 a) = 1 / (1 + exp(-100 a))
__device__ __forceinline__ float softplus100_d(float a) {
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(a * -144.269504088896340736f));
}

// ---- per-point stages: a wave owns 32 points (column j = lane & 31), both wave halves h = lane >> 5 hold the same point ---------------------------

// The point of this lane: its output slot (through the optional index list) and its coordinates, fetched (use_pts) or decoded from the x-major
// lattice linspace(-1,1,R)^3, whose indices the tabulated layer 0 reads.  A dead lane gets slot 0 and a harmless point.
struct TilePoint {
    long long slot;
    float px, py, pz;
    int ix, iy, iz;             // lattice indices (0 with explicit points)
};
__device__ __forceinline__ TilePoint sdf_tile_point(const SdfArgs& a, bool use_pts, long long i, bool live) {
    TilePoint p;
    p.slot = live ? (a.index ? (long long)a.index[i] : i) : 0;
    p.ix = p.iy = p.iz = 0;
    if (use_pts) {
        p.px = live ? a.pts[p.slot * 3 + 0] : 0.f; p.py = live ? a.pts[p.slot * 3 + 1] : 0.f; p.pz = live ? a.pts[p.slot * 3 + 2] : 0.f;
    } else {
        const int R = a.R;
        const unsigned us = (unsigned)p.slot, uR = (unsigned)R;          // R^3 < 2^32: 32-bit divisions (the 64-bit ones cost 240 instructions)
        const unsigned uq = us / uR;
        p.iz = (int)(us - uq * uR); p.ix = (int)(uq / uR); p.iy = (int)(uq - (uq / uR) * uR);
        p.px = lin11(p.ix, R); p.py = lin11(p.iy, R); p.pz = lin11(p.iz, R);
    }
    return p;
}

// this half's 8 channels of one voxel of the channel-last latent volume
__device__ __forceinline__ void latent_voxel(const float* vol_cl, int D, const Taps3D& tp, int dx, int dy, int dz, int h, float (&v)[8]) {
    const size_t vox = ((size_t)tp.ix[dx] * D + tp.iy[dy]) * D + tp.iz[dz];
    const float4* p4 = reinterpret_cast<const float4*>(vol_cl + vox * 16 + 8 * h);
    const float4 v0 = p4[0], v1 = p4[1];
    v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w; v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
}

// trilinear latent, this half's 8 channels: the 8-tap gather with the reference's edge semantics (ops/grid_sampler.py:64-216)
__device__ __forceinline__ void latent_gather(const float* vol_cl, int D, float px, float py, float pz, int h, bool live, float (&lat)[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) lat[c] = 0.f;
    const Taps3D tp = trilinear_ref_taps(px, py, pz, D);
    if (tp.ok && live) {
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dz = 0; dz < 2; ++dz) {
                    float v[8];
                    latent_voxel(vol_cl, D, tp, dx, dy, dz, h, v);
                    const float w = tp.fz[dz] * tp.fy[dy] * tp.fx[dx];
#pragma unroll
                    for (int c = 0; c < 8; ++c) lat[c] = fmaf(v[c], w, lat[c]);
                }
    }
}

// latent path of the gradient: gx += (d sdf / d latent = gl) contracted with the trilinear Jacobian.  The Jacobian is not kept across the network
// (24 registers): the 8 taps are gathered again (L2 hits) and contracted on the fly.
__device__ __forceinline__ void latent_grad(const float* vol_cl, int D, float px, float py, float pz, int h, bool live, const float (&gl)[8], float (&gx)[3]) {
    const Taps3D tp = trilinear_ref_taps(px, py, pz, D);
    if (tp.ok && live) {
        const float half_span = (float)(D - 1) * 0.5f;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dz = 0; dz < 2; ++dz) {
                    float v[8];
                    latent_voxel(vol_cl, D, tp, dx, dy, dz, h, v);
                    float dv = 0.f;
#pragma unroll
                    for (int c = 0; c < 8; ++c) dv = fmaf(v[c], gl[c], dv);
                    gx[0] = fmaf((dx ? half_span : -half_span) * tp.fy[dy] * tp.fz[dz], dv, gx[0]);
                    gx[1] = fmaf((dy ? half_span : -half_span) * tp.fx[dx] * tp.fz[dz], dv, gx[1]);
                    gx[2] = fmaf((dz ? half_span : -half_span) * tp.fx[dx] * tp.fy[dy], dv, gx[2]);
                }
    }
}

// positional encoding (embedder.py:93-101), this half's 20 slots: 0..8 sin of combo 9h+t, 9..17 cos of the same combo, combo c = 3*freq + dim;
// 18: x|z; 19: y|0; N = 24 adds the zero pads that fill the split form's three k steps
template <int N>
__device__ __forceinline__ void pe_half(float px, float py, float pz, int h, float (&pe)[N]) {
    static_assert(N == 20 || N == 24, "20 slots, or 24 with the pads");
    const float p3[3] = {px, py, pz};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int c = 9 * h + t;            // h is wave-half uniform
        const float f = (float)(1 << (c / 3));
        float s, co;
        sincos_pe(p3[t % 3] * f, s, co);    // (9h + t) % 3 == t % 3
        pe[t] = s; pe[9 + t] = co;
    }
    pe[18] = h ? pz : px;
    pe[19] = h ? 0.f : py;
#pragma unroll
    for (int t = 20; t < N; ++t) pe[t] = 0.f;
}

// chain rule through the encoding: gp[0][r] = d/d pe slot r (r < 16), gp[1][0..3] = slots 16..19; pe_at(slot) is the encoding value
// (the fp32 kernel kept it, the split kernel rebuilds it from hi + lo) -> gx = d/d (x, y, z) of this half's slots
template <class PeAt>
__device__ __forceinline__ void pe_chain_rule(const f32x16 (&gp)[2], int h, PeAt pe_at, float (&gx)[3]) {
    gx[0] = gx[1] = gx[2] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int c = 9 * h + t;
        const int d = t % 3;
        const float f = (float)(1 << (c / 3));
        const float gs = gp[0][t];                                  // d/d sin slot
        const float gc = (9 + t < 16) ? gp[0][9 + t] : gp[1][9 + t - 16];
        gx[d] += (gs * pe_at(9 + t) - gc * pe_at(t)) * f;           // sin' = f cos ; cos' = -f sin
    }
    if (h) gx[2] += gp[1][2]; else { gx[0] += gp[1][2]; gx[1] += gp[1][3]; }
}

// accumulators <- bias: misc[off ..] is a MISC row of 128 floats in lane-half order.  Base and offset stay apart: with a pre-offset pointer
// (misc + off) the layer-0 call costs k_sdf_mlp_x3<false> 80 instructions and 8 VGPRs, and k_sdf_mlp<VAR_GRAD> 24 bytes of scratch
template <int NB>
__device__ __forceinline__ void acc_from_bias(f32x16 (&acc)[NB], const float* misc, int off, int h) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = misc[off + (nb * 16 + r) * 2 + h];
}
template <int NB>
__device__ __forceinline__ void acc_zero(f32x16 (&acc)[NB]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
}

// lo in the asm form (split_f16.h): k_sdf_grad_x3 falls below the 256-register line and loses its 224 bytes of scratch per lane, 11.9 -> 9.9 ms on 29.5 M points
constexpr bool MIXLO = true;

// t-domain softplus of four accumulator blocks, split, as the 8 hidden k-step operands of the next layer
__device__ __forceinline__ void softplus_split(const f32x16 (&acc)[4], Split8 (&hb)[8], float m1) {
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        float hv[16];
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const f32x2 sp = softplus_t_pair(f32x2{acc[nb][r], acc[nb][r + 1]});
            hv[r] = sp[0]; hv[r + 1] = sp[1];
        }
        hb[2 * nb] = split8<MIXLO>(hv, 0, m1); hb[2 * nb + 1] = split8<MIXLO>(hv, 8, m1);
    }
}

// value and derivative: returns the SDF row's hidden sum over s' = softplus(a1) * 100 / ln 2 (weights in the MISC_W2H row; SOFTPLUS_INV_SCALE comes off once
// per point) and leaves g1x = d sdf / d a1 = w2row * softplus'(a1), split, as the backward k-step operands (a domain: the backward operands are the
// unscaled ones, weights.py SOFTPLUS_SCALE)
__device__ __forceinline__ float softplus_split_grad(const f32x16 (&acc)[4], const float* misc, int h, Split8 (&g1x)[8], float m1) {
    float yh = 0.f;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        float gv[16];
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            f32x2 d;
            const f32x2 v = softplus_t_pair(f32x2{acc[nb][r], acc[nb][r + 1]}, d);
            const float w2a = misc[MISC_W2H + (nb * 16 + r) * 2 + h], w2b = misc[MISC_W2H + (nb * 16 + r + 1) * 2 + h];
            yh = fmaf(w2a, v[0], yh); yh = fmaf(w2b, v[1], yh);
            gv[r] = w2a * d[0]; gv[r + 1] = w2b * d[1];
        }
        g1x[2 * nb] = split8<MIXLO>(gv, 0, m1); g1x[2 * nb + 1] = split8<MIXLO>(gv, 8, m1);
    }
    return yh;
}

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// A-operand source: an LDS-resident blob segment (plain indexing, ds_read with immediate offsets) or a segment of the
// global blob read through a BUFFER descriptor (wave-uniform rsrc + scalar offset + lane*4): with flat/global loads
// hipcc materialises one 64-bit per-lane address per load site, hoists ~200 of them out of the tile loop and spills them.
struct ASrc {
    const float* lds;
    __amdgpu_buffer_rsrc_t rsrc;
    int base;                 // float offset of the segment in the blob (global case)
};
template <bool GLOBAL>
__device__ __forceinline__ float a_load(const ASrc& s, int idx, int lane) {
    if constexpr (GLOBAL) return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(s.rsrc, lane * 4, (s.base + idx) * 4, 0));
    else return s.lds[idx + lane];
}

// One k-step: acc[nb] += A[nb][step] (x) b for all output blocks.  The A operands of the NEXT step are fetched
// before this step's MFMAs and a scheduling barrier pins that order: without it hipcc hoists hundreds of operand
// loads to the top of the (single, fully unrolled) basic block and spills.
template <int NB, int NST, int N, bool GLOBAL>
__device__ __forceinline__ void mma_run(f32x16 (&acc)[NB], const ASrc& A, int blk0, int lane, int step0, const float (&b)[N]) {
    float cur[NB], nxt[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) cur[nb] = a_load<GLOBAL>(A, ((blk0 + nb) * NST + step0) * 64, lane);
#pragma unroll
    for (int r = 0; r < N; ++r) {
        if (r + 1 < N) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) nxt[nb] = a_load<GLOBAL>(A, ((blk0 + nb) * NST + step0 + r + 1) * 64, lane);
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = MFMA(cur[nb], b[r], acc[nb]);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) cur[nb] = nxt[nb];
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int NB, int NST, bool GLOBAL>
__device__ __forceinline__ void mma_block16(f32x16 (&acc)[NB], const ASrc& A, int lane, int step0, const f32x16& x) {
    float b[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) b[r] = x[r];
    mma_run<NB, NST, 16, GLOBAL>(acc, A, 0, lane, step0, b);
}


// Launch body of the persistent SDF kernels: 512 threads, one tile of 32 points per wave, LDS_FLOATS of dynamic LDS (the layouts above).
template <auto KERNEL, int LDS_FLOATS>
int sdf_launch(const char* what, const SdfArgs& a, void* stream) {
    constexpr int threads = 512;
    constexpr size_t lds_bytes = (size_t)LDS_FLOATS * sizeof(float);
    const unsigned grid = network_grid(a.n, a.n_dev, threads, 32);
    O2345_ENSURE_LDS(KERNEL, lds_bytes);
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(threads), lds_bytes, (hipStream_t)stream, a);
    return check_launch(what);
}

}  // namespace o2345
