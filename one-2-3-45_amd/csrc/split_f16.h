// The split-f16 ("f16x3") operand form of the default numerical mode (config.py), shared by the SDF (sdf_mlp_x3.hip), colour (color_net.h),
// 2-D convolution (convnet.hip) and sparse-convolution (sparse_mfma.hip) kernels.
//
// Every fp32 operand x is split into two f16 halves, x = hi + lo: hi = f16(x) rounded toward zero (two values per v_cvt_pkrtz_f16_f32),
// lo = f16(x - hi) (22 significant bits together; domain |x| < 65504).  A product of two split operands is accumulated in fp32 on
// v_mfma_f32_32x32x16_f16 as lo*hi + hi*lo + hi*hi; the dropped lo*lo term is 2^-22 relative.  gfx950's MFMA honours f16 subnormals and forms
// exact products (checked on hardware).  Weights are split on the host (weights.py), activations in registers by the helpers below.
// The lower end of the domain -- lo is an f16 subnormal below |x| of about 2^-4, its absolute error stops shrinking with x -- is measured and stated in
// DESIGN.md section 4, "split-f16 form: weight scale and accuracy".
//
// lo comes in two forms, identical up to the rounding of the residual (tools/ubench/mixlo_check.hip checks them value by value on hardware):
//   C form (split_pair): x - hi is one v_fma_mix_f32 per value (the f16 operand is converted in flight, exact incl. f16 subnormals -- checked on
//     hardware), then v_cvt_pkrtz: 3 instructions per pair.  The multiplier -1 comes from opaque_minus_one(): with a literal -1 the optimiser
//     rewrites fma(hi, -1, x) into cvt + sub.
//   asm form (split_lo_pair_bits): v_fma_mixlo_f16 / v_fma_mixhi_f16 subtract exactly in fp32 and write the rounded f16 straight into the low /
//     high half of the result: 2 instructions per pair (hipcc does not select them from C code); lo is rounded to nearest instead of toward zero.
#pragma once
#include <hip/hip_runtime.h>

namespace o2345 {

using f32x16 = __attribute__((ext_vector_type(16))) float;
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef __fp16 h16x2 __attribute__((ext_vector_type(2)));        // the type of __builtin_amdgcn_cvt_pkrtz
typedef _Float16 hh16x2 __attribute__((ext_vector_type(2)));
#define MFMA_F16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)

struct Split8 { h16x8 hi, lo; };

__device__ __forceinline__ float opaque_minus_one() {
    float m1 = -1.f;
    asm volatile("" : "+v"(m1));
    return m1;
}

// C form: the halves of the pair (x, y)
__device__ __forceinline__ void split_pair(float x, float y, float m1, h16x2& hi, h16x2& lo) {
    hi = __builtin_amdgcn_cvt_pkrtz(x, y);
    const hh16x2 h = __builtin_bit_cast(hh16x2, hi);
    lo = __builtin_amdgcn_cvt_pkrtz(__builtin_fmaf((float)h[0], m1, x), __builtin_fmaf((float)h[1], m1, y));
}

// C form for ONE value (the other half of both results is zero)
__device__ __forceinline__ void split_one(float x, float m1, _Float16& hi, _Float16& lo) {
    const hh16x2 h = __builtin_bit_cast(hh16x2, __builtin_amdgcn_cvt_pkrtz(x, 0.f));
    hi = h[0];
    lo = __builtin_bit_cast(hh16x2, __builtin_amdgcn_cvt_pkrtz(__builtin_fmaf((float)h[0], m1, x), 0.f))[0];
}

// asm form: the lo halves of the pair (a, b) whose hi halves are packed in `hi_bits`
__device__ __forceinline__ unsigned split_lo_pair_bits(unsigned hi_bits, float a, float b) {
    unsigned lo;
    // `volatile` matters: as a "pure" asm the pair gave wrong colours in k_color_mfma (G < 32) on hardware while s_nop-padded and volatile builds of the same
    // source were correct -- LLVM moves / merges side-effect-free asm in ways the EXEC-ignoring matrix instructions that consume the result do not survive
    asm volatile("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\t"
                 "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
                 : "=&v"(lo) : "v"(hi_bits), "v"(a), "v"(b));
    return lo;
}

// the B operand of the eight values v[s0 .. s0 + 7], zero beyond N (s0 is a compile-time constant after unrolling); MIXLO selects the asm
// form of lo, which does not use m1
template <bool MIXLO = false, int N>
__device__ __forceinline__ Split8 split8(const float (&v)[N], int s0, float m1) {
    union { h16x8 v8; h16x2 v2[4]; } hi, lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float x = (s0 + 2 * i < N) ? v[s0 + 2 * i < N ? s0 + 2 * i : 0] : 0.f;
        const float y = (s0 + 2 * i + 1 < N) ? v[s0 + 2 * i + 1 < N ? s0 + 2 * i + 1 : 0] : 0.f;
        if constexpr (MIXLO) {
            hi.v2[i] = __builtin_amdgcn_cvt_pkrtz(x, y);
            lo.v2[i] = __builtin_bit_cast(h16x2, split_lo_pair_bits(__builtin_bit_cast(unsigned, hi.v2[i]), x, y));
        } else {
            split_pair(x, y, m1, hi.v2[i], lo.v2[i]);
        }
    }
    return {hi.v8, lo.v8};
}

// One k step of NB output blocks, term-major (consecutive matrix instructions go to different accumulators):
// acc[nb] += alo[nb] * b.hi, then += ahi[nb] * b.lo, then += ahi[nb] * b.hi.  No scheduling barrier: callers place their own.
template <int NB>
__device__ __forceinline__ void mfma_x3(f32x16* acc, const h16x8* ahi, const h16x8* alo, const Split8& b) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = MFMA_F16(alo[nb], b.hi, acc[nb]);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = MFMA_F16(ahi[nb], b.lo, acc[nb]);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = MFMA_F16(ahi[nb], b.hi, acc[nb]);
}

// The A operands (weights) of one k step of NB output blocks, as the packers lay them out: [step][block][hi | lo][64 lanes][8 f16], 2 KB per block and
// step, identical for every wave of a grid.  a_fetch streams them from L2 through a buffer descriptor, a_fetch_lds reads a copy staged in LDS.
template <int NB>
struct AOp { h16x8 hi[NB], lo[NB]; };

template <int NB>
__device__ __forceinline__ AOp<NB> a_fetch_lds(const float* wlds, int step, int lane) {
    AOp<NB> r;
    const float4* A = reinterpret_cast<const float4*>(wlds);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        r.hi[nb] = __builtin_bit_cast(h16x8, A[((step * NB + nb) * 2 + 0) * 64 + lane]);
        r.lo[nb] = __builtin_bit_cast(h16x8, A[((step * NB + nb) * 2 + 1) * 64 + lane]);
    }
    return r;
}
template <int NB>
__device__ __forceinline__ AOp<NB> a_fetch(__amdgpu_buffer_rsrc_t rs, int step, int lane) {
    AOp<NB> r;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int base = ((step * NB + nb) * 2) * 1024;          // bytes
        r.hi[nb] = __builtin_bit_cast(h16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, base, 0));
        r.lo[nb] = __builtin_bit_cast(h16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, base + 1024, 0));
    }
    return r;
}

}  // namespace o2345
