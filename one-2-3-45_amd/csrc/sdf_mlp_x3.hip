// SDF network on the f16 matrix cores at fp32-class accuracy ("f16x3" split precision, csrc/split_f16.h).
//
// v_mfma_f32_32x32x2_f32 runs at 1/16 of the f16/bf16 matrix rate, and csrc/sdf_mlp.hip is bound by it.  Here every fp32
// operand is split into f16 halves hi + lo and a product costs three v_mfma_f32_32x32x16_f16 per 16 k instead of eight fp32
// MFMAs: 5.3x less matrix time at ~4e-7 absolute error on O(1) results (the fp32 MFMA chain itself carries ~1e-7).  Weights are
// split on the host (weights.pack_sdf_blob), activations in registers.  Domain: |x| < 65504 (activations here are O(1)).
// Lane layout, blob order and the register chaining between layers: two wave halves supply 8 k values each of a 16-k step (weights.kcol_h / neuron_of).
#include "sdf_common.h"

namespace o2345 {

// acc[ob] += W[ob][step] * b for NB output blocks, split precision.  A: LDS, [NB][NST][hi|lo][64 lanes] float4.
template <int NB, int NST, int B0 = 0, int B1 = NB>
__device__ __forceinline__ void mma_x3_part(f32x16 (&acc)[NB], const float4* A, int lane, int step, const Split8& b) {
    h16x8 ahi[B1 - B0], alo[B1 - B0];
#pragma unroll
    for (int ob = B0; ob < B1; ++ob) {
        ahi[ob - B0] = __builtin_bit_cast(h16x8, A[((ob * NST + step) * 2 + 0) * 64 + lane]);
        alo[ob - B0] = __builtin_bit_cast(h16x8, A[((ob * NST + step) * 2 + 1) * 64 + lane]);
    }
    mfma_x3<B1 - B0>(acc + B0, ahi, alo, b);
    __builtin_amdgcn_sched_barrier(0);
}
template <int NB, int NST>
__device__ __forceinline__ void mma_x3(f32x16 (&acc)[NB], const float4* A, int lane, int step, const Split8& b) {
    if constexpr (NB > 4) {                     // bound the operand registers in flight (8 per block)
        mma_x3_part<NB, NST, 0, 3>(acc, A, lane, step, b);
        mma_x3_part<NB, NST, 3, NB>(acc, A, lane, step, b);
    } else {
        mma_x3_part<NB, NST, 0, NB>(acc, A, lane, step, b);
    }
}

// TAB: the points are the x-major lattice linspace(-1,1,R)^3 (extract_fields) and layer 0 comes from per-axis tables: the positional encoding is
// separable, so W0 . PE(x,y,z) + b0 = Txy[ix,iy] + Tz[iz] -- two 256-byte row reads and 64 adds per lane replace 18 sincos evaluations, the operand
// split of the encoding and the 36 matrix steps of layer 0 (tables in fp64-evaluated fp32: more accurate than the split-f16 products they replace).
template <bool TAB>
__global__ __launch_bounds__(512) void k_sdf_mlp_x3(SdfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int L_A0 = 0, L_A1 = NX_A0, L_MISC = NX_A0 + NX_A1;                 // LDSX_MLP_FLOATS (sdf_common.h)
    for (int i = threadIdx.x * 4; i < L_MISC; i += blockDim.x * 4)                // the two sections are adjacent in the blob
        *reinterpret_cast<float4*>(lds + i) = *reinterpret_cast<const float4*>(a.blob + OFFX_A0 + i);
    for (int i = threadIdx.x; i < MISC_SIZE; i += blockDim.x) lds[L_MISC + i] = a.blob[OFFX_MISC + i];           // b0, b1 in the t domain
    __syncthreads();
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const float m1 = opaque_minus_one();         // not read by the asm form of lo, but dropping it re-allocates the kernel's registers
    const float4* A0 = reinterpret_cast<const float4*>(lds + L_A0);
    const float4* A1 = reinterpret_cast<const float4*>(lds + L_A1);
    const float* misc = lds + L_MISC;

    const long long n = a.n_dev ? (long long)*a.n_dev : a.n;
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const TileSched ts = tile_schedule(n, 32, wave, nwave);
    for (long long tile = ts.first; tile < ts.end; tile += ts.stride) {
        const long long i = tile * 32 + j;
        const bool live = i < n;
        const TilePoint pt = sdf_tile_point(a, !TAB && a.pts, i, live);
        const long long slot = pt.slot;
        float lat[8];
        latent_gather(a.vol_cl, a.D, pt.px, pt.py, pt.pz, h, live, lat);
        f32x16 acc[4];
        if constexpr (TAB) {
            // ---- layer 0 from the tables ------------------------------------------------------------------------------------------------------
            const float4* txy = reinterpret_cast<const float4*>(a.tab_xy + ((size_t)pt.ix * a.R + pt.iy) * 128 + 64 * h);
            const float4* tz = reinterpret_cast<const float4*>(a.tab_z + (size_t)pt.iz * 128 + 64 * h);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 u = txy[nb * 4 + q], w = tz[nb * 4 + q];
                    acc[nb][4 * q] = u.x + w.x; acc[nb][4 * q + 1] = u.y + w.y; acc[nb][4 * q + 2] = u.z + w.z; acc[nb][4 * q + 3] = u.w + w.w;
                }
        } else {
            // ---- layer 0 on the positional encoding (+4 zero pads to fill three k steps) ------------------------------------------------
            float pe[24];
            pe_half(pt.px, pt.py, pt.pz, h, pe);
            acc_from_bias(acc, misc, MISC_B0, h);
#pragma unroll
            for (int s = 0; s < STX0; ++s) mma_x3<4, STX0>(acc, A0, lane, s, split8<MIXLO>(pe, 8 * s, m1));
        }
        Split8 hb[8];                   // softplus(layer 0), split, as the 8 hidden k-step operands of layer 1
        softplus_split(acc, hb, m1);
        // ---- layer 1 -------------------------------------------------------------------------------------------------------------------
        acc_from_bias(acc, misc, MISC_B1, h);
#pragma unroll
        for (int s = 0; s < 8; ++s) mma_x3<4, STH1>(acc, A1, lane, s, hb[s]);
        mma_x3<4, STH1>(acc, A1, lane, 8, split8<MIXLO>(lat, 0, m1));
        // ---- SDF output row: fp32 dot product ------------------------------------------------------------------------------------------
        float yh = 0.f;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const f32x2 sp = softplus_t_pair(f32x2{acc[nb][r], acc[nb][r + 1]});
                yh = fmaf(misc[MISC_W2H + (nb * 16 + r) * 2 + h], sp[0], yh);
                yh = fmaf(misc[MISC_W2H + (nb * 16 + r + 1) * 2 + h], sp[1], yh);
            }
        float y0 = yh * SOFTPLUS_INV_SCALE;          // the hidden activations are s' = softplus * 100 / ln 2: the factor comes off once per point
#pragma unroll
        for (int t = 0; t < 8; ++t) y0 += misc[MISC_W2L + 8 * h + t] * lat[t];
        y0 += __shfl_xor(y0, 32);
        y0 += misc[MISC_B2];
        if (live && h == 0) a.out_sdf[slot] = a.sign * y0;
    }
}


// A operands that do not fit in LDS stream from L2 through a buffer descriptor (wave-uniform base + lane * 16 bytes), fetched
// one phase ahead of their use.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <int NB>
struct AReg { h16x8 hi[NB], lo[NB]; };
template <int NB, int NST>
__device__ __forceinline__ AReg<NB> a_fetch(__amdgpu_buffer_rsrc_t rs, int sec_off_floats, int lane, int blk0, int step) {
    AReg<NB> r;
#pragma unroll
    for (int ob = 0; ob < NB; ++ob) {
        const int base = (sec_off_floats + (((blk0 + ob) * NST + step) * 2) * 256) * 4;      // bytes
        r.hi[ob] = __builtin_bit_cast(h16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, base, 0));
        r.lo[ob] = __builtin_bit_cast(h16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, base + 1024, 0));
    }
    return r;
}

// SDF + analytic gradient (sparse_sdf_network.py:476-499 obtains it with autograd), every product split-f16.
// The four operand blobs are 210 KB together; LDS (160 KB) holds layer 0, layer 1 and output blocks 0-2 of layer 1 transposed
// (146 KB), the remaining 64 KB per tile (blocks 3-4 of layer 1 transposed, layer 0 transposed) stream from L2.
// softplus'(a0) comes from a block-by-block re-evaluation of layer 0 (64 registers otherwise held across the whole network),
// and the trilinear Jacobian is not kept either: the 8 taps are gathered again at the end (L2 hits) and contracted with
// d sdf / d latent on the fly.
__global__ __launch_bounds__(512) void k_sdf_grad_x3(SdfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int L_A0 = 0, L_A1 = NX_A0, L_A1T = NX_A0 + NX_A1, L_MISC = NX_A0 + NX_A1 + NX_A1T3;       // LDSX_GRAD_FLOATS (sdf_common.h)
    for (int i = threadIdx.x * 4; i < L_MISC; i += blockDim.x * 4)                // the three sections are adjacent in the blob
        *reinterpret_cast<float4*>(lds + i) = *reinterpret_cast<const float4*>(a.blob + OFFX_A0 + i);
    for (int i = threadIdx.x; i < MISC_SIZE; i += blockDim.x) lds[L_MISC + i] = a.blob[OFFX_MISC + i];           // b0, b1 in the t domain
    __syncthreads();
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const float m1 = opaque_minus_one();
    const float4* A0 = reinterpret_cast<const float4*>(lds + L_A0);
    const float4* A1 = reinterpret_cast<const float4*>(lds + L_A1);
    const float4* A1T = reinterpret_cast<const float4*>(lds + L_A1T);
    const float* misc = lds + L_MISC;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.blob, 0, BLOB_FLOATS * 4, 0x00020000);

    const long long n = a.n_dev ? (long long)*a.n_dev : a.n;
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const TileSched ts = tile_schedule(n, 32, wave, nwave);
    // every wave of the workgroup runs the same number of iterations (the last one possibly on an empty tile) so that a
    // workgroup barrier before the backward pass keeps the eight waves in step: they then stream the same L2-resident operands
    // (64 KB per tile, twice the L1) at the same time and share each other's L1 fills instead of each re-fetching from L2
    const long long wave0_first = ts.first - wave;
    const long long iters = wave0_first < ts.end ? (ts.end - wave0_first + ts.stride - 1) / ts.stride : 0;
    for (long long it = 0; it < iters; ++it) {
        const long long tile = ts.first + it * ts.stride;
        const long long i = tile * 32 + j;
        const bool live = tile < ts.end && i < n;
        const TilePoint pt = sdf_tile_point(a, a.pts != nullptr, i, live);
        const long long slot = pt.slot;
        const float px = pt.px, py = pt.py, pz = pt.pz;
        // ---- trilinear latent (this half's 8 channels) ----------------------------------------------------------------------------
        Split8 latx;
        float ylat = 0.f;                       // latent part of the SDF output row
        {
            float lat[8];
            latent_gather(a.vol_cl, a.D, px, py, pz, h, live, lat);
#pragma unroll
            for (int t = 0; t < 8; ++t) ylat += misc[MISC_W2L + 8 * h + t] * lat[t];
            latx = split8<MIXLO>(lat, 0, m1);
        }
        // ---- positional encoding: fp32 values (needed again for sin' / cos') and their split form ----------------------------------
        Split8 pex[STX0];
        {
            float pe[24];
            pe_half(px, py, pz, h, pe);
#pragma unroll
            for (int s = 0; s < STX0; ++s) pex[s] = split8<MIXLO>(pe, 8 * s, m1);
        }
        // sin / cos are needed again for the chain rule at the very end; hi + lo reproduces them to 2^-21 (one v_fma_mix_f32 each),
        // which frees the 18 fp32 registers for the whole network
        auto pe_at = [&](int idx) { return (float)pex[idx >> 3].hi[idx & 7] + (float)pex[idx >> 3].lo[idx & 7]; };
        // ---- layer 0 ------------------------------------------------------------------------------------------------------------------------
        f32x16 acc[4];
        acc_from_bias(acc, misc, MISC_B0, h);
#pragma unroll
        for (int s = 0; s < STX0; ++s) mma_x3<4, STX0>(acc, A0, lane, s, pex[s]);
        Split8 hb[8];
        softplus_split(acc, hb, m1);
        // ---- layer 1 ------------------------------------------------------------------------------------------------------------------------
        acc_from_bias(acc, misc, MISC_B1, h);
#pragma unroll
        for (int s = 0; s < 8; ++s) mma_x3<4, STH1>(acc, A1, lane, s, hb[s]);
        mma_x3<4, STH1>(acc, A1, lane, 8, latx);
        AReg<2> tcur = a_fetch<2, STHB>(rs, OFFX_A1T, lane, 3, 0);             // first streamed operands of the backward pass
        Split8 g1x[8];                  // d sdf / d a1 = w2row * softplus'(a1), split, as the backward k-step operands
        const float yh = softplus_split_grad(acc, misc, h, g1x, m1);
        float y0 = fmaf(yh, SOFTPLUS_INV_SCALE, ylat);
        y0 += __shfl_xor(y0, 32);
        y0 += misc[MISC_B2];
        if (live && h == 0) a.out_sdf[slot] = a.sign * y0;
        __syncthreads();                    // align the waves for the streamed phase (see the loop head)
        // ---- backward through layer 1: g[0..3] = d/d h0 (lane layout of h0), g[4][0..7] = d/d latent channel 8h+t ------------------
        f32x16 g[5];
        acc_zero(g);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            // streamed blocks first, then their registers are refilled for the next step while the LDS blocks run (single buffer)
            mfma_x3<2>(g + 3, tcur.hi, tcur.lo, g1x[s]);
            __builtin_amdgcn_sched_barrier(0);
            if (s + 1 < 8) tcur = a_fetch<2, STHB>(rs, OFFX_A1T, lane, 3, s + 1);
            mma_x3_part<5, STHB, 0, 3>(g, A1T, lane, s, g1x[s]);
        }
        // ---- backward through layer 0: softplus'(a0) from a block-by-block re-evaluation; transposed operands streamed -------------
        f32x16 gp[2];
        acc_zero(gp);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const AReg<2> ta = a_fetch<2, STHB>(rs, OFFX_A0T, lane, 0, 2 * nb);
            __builtin_amdgcn_sched_barrier(0);
            f32x16 a0r[1];
            acc_from_bias(a0r, misc, MISC_B0 + nb * 32, h);
#pragma unroll
            for (int s = 0; s < STX0; ++s) mma_x3_part<1, STX0, 0, 1>(a0r, A0 + nb * STX0 * 2 * 64, lane, s, pex[s]);
            const AReg<2> tb = a_fetch<2, STHB>(rs, OFFX_A0T, lane, 0, 2 * nb + 1);     // covered by the softplus' block and ta's MFMAs
            __builtin_amdgcn_sched_barrier(0);
            float gv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) gv[r] = g[nb][r] * softplus_t_d(a0r[0][r]);
            mfma_x3<2>(gp, ta.hi, ta.lo, split8<MIXLO>(gv, 0, m1));
            mfma_x3<2>(gp, tb.hi, tb.lo, split8<MIXLO>(gv, 8, m1));
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- chain rule through the encoding, then the latent path -----------------------------------------------------------------------
        float gx[3], gl[8];
        pe_chain_rule(gp, h, pe_at, gx);
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

// Pre-pass of the sparse lattice evaluation (o2345_sdf_grid_sparse_x3): one lane per lattice point, 32 lanes per tile.  A tile none of whose points is
// active (geom_math.h grid_point_active) gets out = sign * background; the slots of every other tile are appended to `index`, 32 per tile, and
// *n_active (zeroed by the launcher) counts them -- the per-point list and device-side count that k_sdf_mlp_x3 already takes.  A workgroup owns
// GRID_CHUNK_TILES consecutive tiles and reserves its stretch of the list with ONE atomic; the order of the stretches is free, results are scattered by
// slot.  The pad lanes of a partial last tile repeat the last slot: the same point, evaluated to the same value, stored to the same address.
constexpr int GRID_CHUNK_TILES = 256;     // = threads per workgroup: the compaction gives every tile of the chunk one thread
constexpr size_t GRID_WS_HEAD = 256;      // workspace: the count (int32) in a block of its own, then the list
static_assert(GRID_TILE == 32 && GRID_CHUNK_TILES % 64 == 0, "a tile is one half of a wave, as in k_sdf_mlp_x3");
__global__ __launch_bounds__(GRID_CHUNK_TILES) void k_grid_active_tiles(const float* __restrict__ maskvol, int D, int R, const float* __restrict__ background,
                                                                        float sign, float* __restrict__ out, int32_t* __restrict__ index, int32_t* n_active) {
    __shared__ int s_active[GRID_CHUNK_TILES], s_list[GRID_CHUNK_TILES], s_wave[GRID_CHUNK_TILES / 64 + 1], s_base;
    const long long n = (long long)R * R * R;
    const long long tile0 = (long long)blockIdx.x * GRID_CHUNK_TILES;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    for (int it = 0; it < GRID_CHUNK_TILES / 8; ++it) {
        const int t = it * 8 + wave * 2 + half;                       // tile of the chunk: two per wave and iteration
        const long long slot = (tile0 + t) * GRID_TILE + (lane & 31);
        const bool live = slot < n;
        const unsigned long long b = __ballot(live && grid_point_active(slot, R, D, maskvol));
        const bool tile_active = (half ? (b >> 32) : (b & 0xffffffffull)) != 0;
        if (live && !tile_active) out[slot] = sign * background[slot];
        if ((lane & 31) == 0) s_active[t] = tile_active;
    }
    __syncthreads();
    const bool mine = s_active[threadIdx.x] != 0;
    int total;
    const int pos = block_prefix<GRID_CHUNK_TILES / 64>(mine, s_wave, total);
    if (mine) s_list[pos] = threadIdx.x;
    if (threadIdx.x == 0) s_base = total ? atomicAdd(n_active, total * GRID_TILE) : 0;
    __syncthreads();
    const int base = s_base;
    for (int e = threadIdx.x; e < total * GRID_TILE; e += GRID_CHUNK_TILES) {
        const long long slot = (tile0 + s_list[e >> 5]) * GRID_TILE + (e & 31);
        index[base + e] = (int32_t)(slot < n ? slot : n - 1);
    }
}

}  // namespace o2345

using namespace o2345;

extern "C" {

// argument check shared by the three split-f16 entry points
static int sdf_x3_check(const char* what, bool pointers, int D, bool has_pts, int grid_R) {
    O2345_REQUIRE(pointers, "%s: null pointer", what);
    O2345_REQUIRE(D >= 2, "%s: bad volume side %d", what, D);
    O2345_REQUIRE(has_pts || (grid_R >= 2 && grid_R <= 1600), "%s: need points or a grid resolution in [2, 1600]", what);
    return 0;
}

int o2345_sdf_grad_x3(const float* blob, const float* vol_cl, int D, const float* pts, const int32_t* index, const int32_t* n_dev,
                      long long n, int grid_R, float sign, float* out_sdf, float* out_grad, void* stream) {
    if (const int rc = sdf_x3_check("sdf_grad_x3", blob && vol_cl && out_sdf && out_grad, D, pts, grid_R)) return rc;
    if (n <= 0 && !n_dev) return 0;
    const SdfArgs a{blob, vol_cl, D, pts, index, n_dev, n, grid_R, sign, out_sdf, nullptr, nullptr, out_grad, nullptr};
    return sdf_launch<k_sdf_grad_x3, LDSX_GRAD_FLOATS>("sdf_grad_x3", a, stream);
}

int o2345_sdf_mlp_x3(const float* blob, const float* vol_cl, int D, const float* pts, const int32_t* index, const int32_t* n_dev,
                     long long n, int grid_R, float sign, float* out_sdf, void* stream) {
    if (const int rc = sdf_x3_check("sdf_mlp_x3", blob && vol_cl && out_sdf, D, pts, grid_R)) return rc;
    if (n <= 0 && !n_dev) return 0;
    const SdfArgs a{blob, vol_cl, D, pts, index, n_dev, n, grid_R, sign, out_sdf, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return sdf_launch<k_sdf_mlp_x3<false>, LDSX_MLP_FLOATS>("sdf_mlp_x3", a, stream);
}

// tab_xy[(ix * R + iy)][c] = tab_axes[0][ix][c] + tab_axes[1][iy][c] + bias[c]   (c = 128 lane-ordered columns; summed in doubles)
__global__ __launch_bounds__(128) void k_sdf_tab_xy(const float* __restrict__ axes /*[3][R][128]*/, const float* __restrict__ bias /*[128]*/, int R,
                                                     float* __restrict__ tab_xy) {
    const int c = threadIdx.x, ix = blockIdx.x / R, iy = blockIdx.x % R;
    tab_xy[(size_t)blockIdx.x * 128 + c] = (float)((double)axes[(size_t)ix * 128 + c] + (double)axes[((size_t)R + iy) * 128 + c] + (double)bias[c]);
}

int o2345_sdf_grid_tables(const float* tab_axes, const float* bias_lane_order, int grid_R, float* tab_xy, void* stream) {
    O2345_REQUIRE(tab_axes && bias_lane_order && tab_xy && grid_R >= 2 && grid_R <= 1600, "sdf_grid_tables: bad arguments");
    hipLaunchKernelGGL(k_sdf_tab_xy, dim3(grid_R * grid_R), dim3(128), 0, (hipStream_t)stream, tab_axes, bias_lane_order, grid_R, tab_xy);
    return check_launch("sdf_grid_tables");
}

// extract_fields (sparse_neus_renderer.py:881-905) with layer 0 of the SDF network read from per-axis tables: out_sdf[R^3] = sign * sdf on the
// x-major lattice linspace(-1,1,R)^3.  tab_xy [R*R,128] from o2345_sdf_grid_tables, tab_z [R,128] = the z table (tab_axes + 2*R*128).
int o2345_sdf_grid_x3(const float* blob, const float* vol_cl, int D, int grid_R, float sign, const float* tab_xy, const float* tab_z, float* out_sdf,
                      void* stream) {
    if (const int rc = sdf_x3_check("sdf_grid_x3", blob && vol_cl && out_sdf && tab_xy && tab_z, D, false, grid_R)) return rc;
    const long long n = (long long)grid_R * grid_R * grid_R;
    const SdfArgs a{blob, vol_cl, D, nullptr, nullptr, nullptr, n, grid_R, sign, out_sdf, nullptr, nullptr, nullptr, nullptr, tab_xy, tab_z};
    return sdf_launch<k_sdf_mlp_x3<true>, LDSX_MLP_FLOATS>("sdf_grid_x3", a, stream);
}

size_t o2345_sdf_grid_sparse_workspace_bytes(int grid_R) {
    if (grid_R < 2 || (long long)grid_R * grid_R * grid_R >= (1ll << 31)) return 0;
    const long long ntiles = ((long long)grid_R * grid_R * grid_R + GRID_TILE - 1) / GRID_TILE;
    return GRID_WS_HEAD + (size_t)ntiles * GRID_TILE * sizeof(int32_t);
}

// o2345_sdf_grid_x3 evaluated only where the scene has a latent (the caller's two guarantees: include/o2345.h).  An inactive point samples a latent of
// exactly zero: the latent k-step and the W2L dot product of k_sdf_mlp_x3 add exact zeros, so its value is the background's, and sign = -1 is an exact
// negation.  Every other 32-slot tile goes through k_sdf_mlp_x3<true> with the same inputs as in o2345_sdf_grid_x3: out_sdf is that entry's bit for bit.
int o2345_sdf_grid_sparse_x3(const float* blob, const float* vol_cl, const float* maskvol, int D, int grid_R, float sign, const float* tab_xy,
                             const float* tab_z, const float* background, float* out_sdf, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = sdf_x3_check("sdf_grid_sparse_x3", blob && vol_cl && maskvol && background && out_sdf && tab_xy && tab_z && workspace, D, false, grid_R))
        return rc;
    const long long n = (long long)grid_R * grid_R * grid_R;
    O2345_REQUIRE(n < (1ll << 31), "sdf_grid_sparse_x3: grid_R^3 must stay below 2^31 (got %d)", grid_R);
    O2345_REQUIRE(workspace_bytes >= o2345_sdf_grid_sparse_workspace_bytes(grid_R) && ((uintptr_t)workspace & 15) == 0,
                  "sdf_grid_sparse_x3: workspace too small or misaligned");
    int32_t* n_active = reinterpret_cast<int32_t*>(workspace);
    int32_t* index = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + GRID_WS_HEAD);
    O2345_HIP(hipMemsetAsync(n_active, 0, sizeof(int32_t), (hipStream_t)stream));
    const long long ntiles = (n + GRID_TILE - 1) / GRID_TILE;
    hipLaunchKernelGGL(k_grid_active_tiles, dim3(cdiv(ntiles, GRID_CHUNK_TILES)), dim3(256), 0, (hipStream_t)stream, maskvol, D, grid_R, background, sign,
                       out_sdf, index, n_active);
    if (const int rc = check_launch("sdf_grid_sparse_x3 (active tiles)")) return rc;
    const SdfArgs a{blob, vol_cl, D, nullptr, index, n_active, n, grid_R, sign, out_sdf, nullptr, nullptr, nullptr, nullptr, tab_xy, tab_z};
    return sdf_launch<k_sdf_mlp_x3<true>, LDSX_MLP_FLOATS>("sdf_grid_sparse_x3", a, stream);
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_sdf_mlp_x3() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)(k_sdf_grad_x3));
}
}  // namespace o2345
