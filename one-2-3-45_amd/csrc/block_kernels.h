// Small non-matrix kernels and block-level steps shared by several translation units (costvol.hip, sparse.hip, convnet.hip, and through
// mesh_common.h, which adds what only the mesh units share, mcubes.hip, mesh_components.hip, mesh_smooth.hip, mesh_decimate.hip).
// The kernels live in an anonymous namespace: every unit that launches one instantiates its own copy in its own code object, so o2345_preload
// and the runtime's per-unit loading see them as before.
#pragma once
#include "common.h"

namespace o2345 {

constexpr int IDX_BLOCK = 256;          // threads per block of the index / compaction kernels

// fixed-order sum of (s, q) over a 256-thread block: wave butterflies, then (w0 + w1) + (w2 + w3) -- deterministic.  Returns true in thread 0,
// which then holds the block sums; the other threads return false and must not use s, q.
__device__ __forceinline__ bool block_sum2_256(double& s, double& q) {
    __shared__ double sm[2][4];
    for (int off = 32; off; off >>= 1) { s += __shfl_xor(s, off); q += __shfl_xor(q, off); }
    if ((threadIdx.x & 63) == 0) { sm[0][threadIdx.x >> 6] = s; sm[1][threadIdx.x >> 6] = q; }
    __syncthreads();
    if (threadIdx.x != 0) return false;
    s = (sm[0][0] + sm[0][1]) + (sm[0][2] + sm[0][3]);
    q = (sm[1][0] + sm[1][1]) + (sm[1][2] + sm[1][3]);
    return true;
}

// block-wide exclusive scan of one int per thread (256 threads); lds is free again on return: mcubes.hip, mesh_components.hip
__device__ __forceinline__ int block_scan_excl(int v, int* lds /*[5]*/, int& total) {
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int t = __shfl_up(inc, off);
        if ((threadIdx.x & 63) >= off) inc += t;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) lds[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { int t = lds[i]; if (i < w) base += t; tot += t; }
    total = tot;
    __syncthreads();
    return base + inc - v;
}

// ascending bitonic network over N registers (N a power of two; every index is a compile-time constant after unrolling): mesh_smooth.hip, mesh_decimate.hip
__device__ __forceinline__ void regs_cmpswap(int& x, int& y) {
    const int lo = min(x, y), hi = max(x, y);
    x = lo; y = hi;
}

template <int N>
__device__ __forceinline__ void sort_regs(int (&r)[N]) {
#pragma unroll
    for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    if ((i & k) == 0) regs_cmpswap(r[i], r[l]);
                    else regs_cmpswap(r[l], r[i]);
                }
            }
        }
    }
}

// batch statistics of channel c -> the (scale, shift) pair of InPlaceABN: s = sum x, q = sum x^2 over `count` values, biased variance;
// abs_gamma selects the |gamma| + eps convention of inplace_abn; (mean, var) also go to mean_var when it is not null
__device__ __forceinline__ void abn_scale_shift(double s, double q, double count, int c, int C, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, float eps, int abs_gamma, float* __restrict__ scale_shift,
                                                float* __restrict__ mean_var = nullptr) {
    const double mean = s / count;
    double var = q / count - mean * mean;
    if (var < 0.0) var = 0.0;
    float g = gamma[c];
    if (abs_gamma) g = fabsf(g) + eps;
    const float inv = (float)(1.0 / sqrt(var + (double)eps));
    scale_shift[c] = g * inv;
    scale_shift[C + c] = beta[c] - (float)mean * g * inv;
    if (mean_var) { mean_var[c] = (float)mean; mean_var[C + c] = (float)var; }
}

// A producer's InPlaceABN applied by its consumer on load: leaky ReLU of t = x * scale + shift, in the two spellings the library's kernels were written
// with.  For 0 <= slope < 1 (every caller: 0 or 0.01) they agree in value on every non-NaN t, signed zeros included: t >= 0 gives t * slope <= t with
// the product keeping t's sign, t < 0 gives t * slope >= t.  They compile to different instructions (v_mul + v_max against v_cmp + v_mul + v_cndmask),
// so each site keeps the one it was tuned with.
__device__ __forceinline__ float abn_act_max(float x, float scale, float shift, float slope) {        // the matrix-core convolutions' staging
    const float t = x * scale + shift;
    return fmaxf(t, t * slope);
}
__device__ __forceinline__ float abn_act_select(float x, float scale, float shift, float slope) {     // the fp32 kernels
    const float t = x * scale + shift;
    return t >= 0.f ? t : t * slope;
}

namespace {

// exclusive scan of n ints in place by ONE 1024-thread block (n <= a few 100k block totals); *total = the sum
template <typename Total>
__global__ __launch_bounds__(1024) void k_scan_small(int* __restrict__ a, int n, Total* __restrict__ total) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int lo = t * per, hi = min(n, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += a[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {       // Hillis-Steele inclusive scan over the 1024 partials
        int v = (t >= off) ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int i = lo; i < hi; ++i) {
        int v = a[i];
        a[i] = run;
        run += v;
    }
    if (t == 1023) *total = (Total)part[1023];
}

// exclusive scan of a long int array in three launches: k_tile_sum (one block per tile of 256 * ITEMS entries -> block_total), k_scan_small over the block
// totals, k_tile_scan (block_base = the scanned block totals) -> out[i], and out2[i] when that is not null.  Launched by exclusive_scan (mesh_common.h)
template <int ITEMS>
__global__ __launch_bounds__(256) void k_tile_sum(const int* __restrict__ a, long long n, int* __restrict__ block_total) {
    __shared__ int lds[5];
    const long long i0 = (long long)blockIdx.x * (IDX_BLOCK * ITEMS) + threadIdx.x;
    int s = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) s += (i0 + k * 256 < n) ? a[i0 + k * 256] : 0;
    int total;
    (void)block_scan_excl(s, lds, total);
    if (threadIdx.x == 0) block_total[blockIdx.x] = total;
}

template <int ITEMS>
__global__ __launch_bounds__(256) void k_tile_scan(const int* __restrict__ a, long long n, const int* __restrict__ block_base, int* __restrict__ out,
                                                   int* __restrict__ out2) {
    __shared__ int lds[5];
    const long long i0 = (long long)blockIdx.x * (IDX_BLOCK * ITEMS) + threadIdx.x;
    int run = block_base[blockIdx.x];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const long long i = i0 + k * 256;
        const int x = i < n ? a[i] : 0;
        int total;
        const int at = run + block_scan_excl(x, lds, total);
        if (i < n) {
            out[i] = at;
            if (out2) out2[i] = at;
        }
        run += total;
    }
}

// [V,C,HW] -> [V,HW,C] through a 64-pixel x C LDS tile (coalesced reads and writes).  ACT: y = leaky_relu(x * ss[c] + ss[C + c], slope) on the
// way, also written in NCHW to y_nchw when that is not null; y_nhwc may be null then.
template <int C, bool ACT>
__global__ __launch_bounds__(256) void k_nchw_to_nhwc(const float* __restrict__ x, const float* __restrict__ ss, float slope, int HW,
                                                      float* __restrict__ y_nchw, float* __restrict__ y_nhwc) {
    __shared__ float tile[C][65];
    const int v = blockIdx.y, p0 = blockIdx.x * 64;
    const float* src = x + (size_t)v * C * HW;
    for (int i = threadIdx.x; i < C * 64; i += 256) {
        const int c = i / 64, p = i % 64;
        float t = 0.f;
        if (p0 + p < HW) {
            t = src[(size_t)c * HW + p0 + p];
            if (ACT) {
                t = abn_act_select(t, ss[c], ss[C + c], slope);
                if (y_nchw) y_nchw[((size_t)v * C + c) * HW + p0 + p] = t;
            }
        }
        tile[c][p] = t;
    }
    if (!y_nhwc) return;
    __syncthreads();
    float* dst = y_nhwc + (size_t)v * HW * C;
    for (int i = threadIdx.x; i < C * 64; i += 256) {
        const int p = i / C, c = i % C;
        if (p0 + p < HW) dst[(size_t)(p0 + p) * C + c] = tile[c][p];
    }
}

// launches k_nchw_to_nhwc<C, ACT> for the runtime channel count C, one of C0, Cs... (the caller has checked it; the last one is the fallback)
template <bool ACT, int C0, int... Cs>
void launch_nchw_to_nhwc(int C, const float* x, const float* ss, float slope, int V, long long HW, float* y_nchw, float* y_nhwc, hipStream_t s) {
    if constexpr (sizeof...(Cs) > 0) {
        if (C != C0) return launch_nchw_to_nhwc<ACT, Cs...>(C, x, ss, slope, V, HW, y_nchw, y_nhwc, s);
    }
    hipLaunchKernelGGL((k_nchw_to_nhwc<C0, ACT>), dim3(cdiv(HW, 64), V), dim3(256), 0, s, x, ss, slope, (int)HW, y_nchw, y_nhwc);
}

}  // namespace
}  // namespace o2345
