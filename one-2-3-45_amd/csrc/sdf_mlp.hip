// SDF network evaluation on MFMA: trilinear latent gather (reference edge
// semantics, ops/grid_sampler.py:64-216) + positional encoding (embedder.py:93-101) + LatentSDFLayer
// (sparse_sdf_network.py:35-136: 39->128 softplus, [128|16]->128 softplus, [128|16]->128) and, optionally, the
// analytic input gradient that the reference obtains with autograd (sparse_sdf_network.py:476-499).
//
// Mapping (fp32-exact path, v_mfma_f32_32x32x2_f32 = exact fp32 FMA chain at the fp32 vector rate):
//   D[neuron][point] = sum_k W[neuron][k] * X[k][point]   -- A = weights, B = activations.
//   A wave owns 32 points (B column j = lane & 31); both wave halves h = lane >> 5 hold the same point and supply
//   the two k rows of each 32x32x2 step.  The MFMA result layout puts neuron n = 32*nb + (r&3) + 8*(r>>2) + 4*h in
//   register r of accumulator block nb of half h -- and that is exactly the (k, half) enumeration we use for the NEXT
//   layer's steps, so hidden activations never leave registers: no LDS transpose, no cross-lane traffic.  The price
//   is paid once on the host: weights are pre-permuted into "A blobs" [block][step][64 lanes] (weights.py).
//   Latent channels are split 8|8 and PE entries 20|20 between the halves the same way.
//   Weight blobs for the wide layers live in LDS (persistent workgroups, one per CU); the small ones stream from L2.
#include "sdf_common.h"

namespace o2345 {

template <int VARIANT>
__global__ __launch_bounds__(512) void k_sdf_mlp(SdfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // ---- stage the wide-layer blobs in LDS (layout: sdf_common.h) ---------------------------------------------------
    constexpr int L_FIRST = sdf_lds_first(VARIANT), L_SECOND = sdf_lds_second(VARIANT);
    {
        const float* src1 = a.blob + (VARIANT == VAR_SDF ? OFF_A0 : OFF_A1);
        const float* src2 = a.blob + (VARIANT == VAR_SDF ? OFF_A1 : (VARIANT == VAR_FULL ? OFF_A2 : OFF_A1T));
        for (int i = threadIdx.x * 4; i < L_FIRST; i += blockDim.x * 4)
            *reinterpret_cast<float4*>(lds + i) = *reinterpret_cast<const float4*>(src1 + i);
        for (int i = threadIdx.x * 4; i < L_SECOND; i += blockDim.x * 4)
            *reinterpret_cast<float4*>(lds + L_FIRST + i) = *reinterpret_cast<const float4*>(src2 + i);
        for (int i = threadIdx.x; i < MISC_SIZE; i += blockDim.x) lds[L_FIRST + L_SECOND + i] = a.blob[OFF_MISC + i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    constexpr bool A0G = VARIANT != VAR_SDF;                    // layer-0 blob streams from L2 except in the SDF-only variant
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.blob, 0, BLOB_FLOATS * 4, 0x00020000);
    const ASrc A0{VARIANT == VAR_SDF ? lds : nullptr, rs, OFF_A0};
    const ASrc A1{VARIANT == VAR_SDF ? lds + N_A0 : lds, rs, 0};
    const ASrc A2{lds + N_A1, rs, 0};                          // VAR_FULL only
    const ASrc A1T{lds + N_A1, rs, 0};                         // VAR_GRAD only
    const ASrc A0T{nullptr, rs, OFF_A0T};                      // VAR_GRAD only (L2 resident)
    const float* misc = lds + L_FIRST + L_SECOND;

    const long long n = a.n_dev ? (long long)*a.n_dev : a.n;
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const TileSched ts = tile_schedule(n, 32, wave, nwave);
    for (long long tile = ts.first; tile < ts.end; tile += ts.stride) {
        const long long i = tile * 32 + j;
        const bool live = i < n;
        const TilePoint pt = sdf_tile_point(a, a.pts != nullptr, i, live);
        const long long slot = pt.slot;
        const float px = pt.px, py = pt.py, pz = pt.pz;
        // ---- trilinear latent (this half's 8 channels), or the caller's ---------------------------------------------
        float lat[8];
        if (a.lat_in) {
#pragma unroll
            for (int c = 0; c < 8; ++c) lat[c] = 0.f;
            if (live) {
                const float4* p4 = reinterpret_cast<const float4*>(a.lat_in + slot * 16 + 8 * h);
                const float4 v0 = p4[0], v1 = p4[1];
                lat[0] = v0.x; lat[1] = v0.y; lat[2] = v0.z; lat[3] = v0.w; lat[4] = v1.x; lat[5] = v1.y; lat[6] = v1.z; lat[7] = v1.w;
            }
        } else {
            latent_gather(a.vol_cl, a.D, px, py, pz, h, live, lat);
        }
        float pe[20];
        pe_half(px, py, pz, h, pe);

        // ---- layer 0 ---------------------------------------------------------------------------------------------------
        f32x16 acc[4];
        acc_from_bias(acc, misc, MISC_B0, h);
        mma_run<4, ST0, 20, A0G>(acc, A0, 0, lane, 0, pe);
        f32x16 h0[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const f32x2 sp = softplus100_pair(f32x2{acc[nb][r], acc[nb][r + 1]});
                h0[nb][r] = sp[0]; h0[nb][r + 1] = sp[1];
            }

        // ---- layer 1 ---------------------------------------------------------------------------------------------------
        acc_from_bias(acc, misc, MISC_B1, h);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) mma_block16<4, ST1, false>(acc, A1, lane, kb * 16, h0[kb]);
        mma_run<4, ST1, 8, false>(acc, A1, 0, lane, 64, lat);
        f32x16 h1[4];
        // g1 = d sdf / d a1 = w2row * softplus'(a1)  (kept in place of s1)
        f32x16 g1[4];
        float y0 = 0.f;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                f32x2 d;
                const f32x2 v = (VARIANT == VAR_GRAD) ? softplus100_pair(f32x2{acc[nb][r], acc[nb][r + 1]}, d)
                                                      : softplus100_pair(f32x2{acc[nb][r], acc[nb][r + 1]});
                h1[nb][r] = v[0]; h1[nb][r + 1] = v[1];
                const float w2a = misc[MISC_W2H + (nb * 16 + r) * 2 + h], w2b = misc[MISC_W2H + (nb * 16 + r + 1) * 2 + h];
                y0 = fmaf(w2a, v[0], y0); y0 = fmaf(w2b, v[1], y0);
                if (VARIANT == VAR_GRAD) { g1[nb][r] = w2a * d[0]; g1[nb][r + 1] = w2b * d[1]; }
            }
        // ---- output layer ------------------------------------------------------------------------------------------------
        if (VARIANT == VAR_FULL) {
            acc_from_bias(acc, misc, MISC_B2, h);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) mma_block16<4, ST1, false>(acc, A2, lane, kb * 16, h1[kb]);
            mma_run<4, ST1, 8, false>(acc, A2, 0, lane, 64, lat);
            if (live) {
                if (a.out_feat) {
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            a.out_feat[slot * 128 + nb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = acc[nb][r];
                }
                if (h == 0) a.out_sdf[slot] = a.sign * acc[0][0];      // neuron 0 sits in (nb 0, r 0, h 0)
            }
        } else {
#pragma unroll
            for (int t = 0; t < 8; ++t) y0 += misc[MISC_W2L + 8 * h + t] * lat[t];
            y0 += __shfl_xor(y0, 32);
            y0 += misc[MISC_B2];                                         // b2[0] is slot (nb 0, r 0, h 0)
            if (live && h == 0) a.out_sdf[slot] = a.sign * y0;
        }
        if (a.out_lat && live) {
            float4* o = reinterpret_cast<float4*>(a.out_lat + slot * 16 + 8 * h);
            o[0] = make_float4(lat[0], lat[1], lat[2], lat[3]);
            o[1] = make_float4(lat[4], lat[5], lat[6], lat[7]);
        }
        // ---- backward: d sdf / d x ----------------------------------------------------------------------------------------
        if (VARIANT == VAR_GRAD) {
            f32x16 g[5];
            acc_zero(g);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) mma_block16<5, STB, false>(g, A1T, lane, kb * 16, g1[kb]);
            // g[0..3] = d/d h0 (same lane layout as h0) ; g[4][0..7] = d/d latent channel 8h+t (through layer 1)
            // softplus'(a0) is needed here, 700 MFMAs after layer 0 ran.  Keeping it would cost 64 registers across the whole
            // kernel (and a second wave per SIMD); re-running layer 0 block by block costs 80 cheap MFMAs (+10 %).
            f32x16 g0[4];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                f32x16 a0r[1];
                acc_from_bias(a0r, misc, MISC_B0 + nb * 32, h);
                mma_run<1, ST0, 20, A0G>(a0r, A0, nb, lane, 0, pe);
#pragma unroll
                for (int r = 0; r < 16; ++r) g0[nb][r] = g[nb][r] * softplus100_d(a0r[0][r]);
            }
            f32x16 gp[2];
            acc_zero(gp);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) mma_block16<2, STB, true>(gp, A0T, lane, kb * 16, g0[kb]);
            float gx[3], gl[8];
            pe_chain_rule(gp, h, [&](int slot_) { return pe[slot_]; }, gx);
#pragma unroll
            for (int t = 0; t < 8; ++t) gl[t] = g[4][t] + misc[MISC_W2L + 8 * h + t];
            latent_grad(a.vol_cl, a.D, px, py, pz, h, live, gl, gx);
#pragma unroll
            for (int d = 0; d < 3; ++d) gx[d] += __shfl_xor(gx[d], 32);
            if (live && h == 0 && a.out_grad) {
                a.out_grad[slot * 3 + 0] = gx[0]; a.out_grad[slot * 3 + 1] = gx[1]; a.out_grad[slot * 3 + 2] = gx[2];
            }
        }
    }
}

}  // namespace o2345

using namespace o2345;

extern "C" {

int o2345_sdf_blob_floats(void) { return BLOB_FLOATS; }

int o2345_sdf_mlp_ex(int variant, const float* blob, const float* vol_cl, int D, const float* pts, const int32_t* index,
                     const int32_t* n_dev, long long n, int grid_R, float sign, const float* lat_in, float* out_sdf,
                     float* out_feat, float* out_lat, float* out_grad, void* stream);

// variant: 0 = SDF only, 1 = all 128 outputs (+SDF), 2 = SDF + analytic gradient
int o2345_sdf_mlp(int variant, const float* blob, const float* vol_cl, int D, const float* pts, const int32_t* index,
                  const int32_t* n_dev, long long n, int grid_R, float sign, float* out_sdf, float* out_feat,
                  float* out_lat, float* out_grad, void* stream) {
    return o2345_sdf_mlp_ex(variant, blob, vol_cl, D, pts, index, n_dev, n, grid_R, sign, nullptr, out_sdf, out_feat, out_lat, out_grad, stream);
}

int o2345_sdf_mlp_ex(int variant, const float* blob, const float* vol_cl, int D, const float* pts, const int32_t* index,
                     const int32_t* n_dev, long long n, int grid_R, float sign, const float* lat_in, float* out_sdf,
                     float* out_feat, float* out_lat, float* out_grad, void* stream) {
    O2345_REQUIRE(blob && (vol_cl || lat_in) && out_sdf, "sdf_mlp: null pointer");
    O2345_REQUIRE(!lat_in || (variant != VAR_GRAD && pts), "sdf_mlp: lat_in needs explicit points and no gradient");
    O2345_REQUIRE(D >= 2, "sdf_mlp: bad volume side %d", D);
    O2345_REQUIRE(pts || (grid_R >= 2 && grid_R <= 1600), "sdf_mlp: need points or a grid resolution in [2, 1600]");
    O2345_REQUIRE(variant >= 0 && variant <= 2, "sdf_mlp: bad variant %d", variant);
    O2345_REQUIRE(variant != VAR_GRAD || out_grad, "sdf_mlp: gradient variant needs out_grad");
    if (n <= 0 && !n_dev) return 0;
    const SdfArgs a{blob, vol_cl, D, pts, index, n_dev, n, grid_R, sign, out_sdf, out_feat, out_lat, out_grad, lat_in};
#define O2345_SDF_VARIANT(V) sdf_launch<k_sdf_mlp<V>, sdf_lds_floats(V)>
    static int (*const launch[3])(const char*, const SdfArgs&, void*) = {O2345_SDF_VARIANT(VAR_SDF), O2345_SDF_VARIANT(VAR_FULL), O2345_SDF_VARIANT(VAR_GRAD)};
#undef O2345_SDF_VARIANT
    return launch[variant]("sdf_mlp", a, stream);
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_sdf_mlp() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)(k_sdf_mlp<0>));
}
}  // namespace o2345
