// Hierarchical ray sampling + NeuS compositing: SparseNeuSRenderer.render
// (models/sparse_neus_renderer.py:457-635) with up_sample (:73-115), cat_z_vals (:117-151), render_core (:171-455).
//
// The reference runs ~40 small kernels per up-sampling round per 512-ray chunk.  Here one lane owns one ray; all
// per-ray lists are sample-major ([S][R]) so every access of the wave is a coalesced row segment; the SDF network
// is called on flat point lists (occupied points compacted with a ballot/popcount prefix into an index list that
// the MFMA kernel consumes with a device-side count -- no host synchronisation anywhere in a render call).
#include "common.h"                    // pulls in include/o2345.h: O2345RenderIO is declared THERE only (layout-checked by the binding at load time)
#include "render_math.h"

namespace o2345 {

// The device-side counters of one render call (ints in the workspace, RenderLayout::counters), cleared by the call's first kernel (k_ray_coarse).
enum RenderCounter {
    RC_ROUND = 0,       // + i, i < 4: list entries of up-sampling round i (the new samples inside the mask)
    RC_FINAL = 4,       // list entries of the finalize round (the occupied mid-points)
    RC_CULLED = 5,      // entries of the weight-culled list (k_ray_cull)
    RC_DONE = 8,        // + i, i < 5: finished workgroups of round i (4 = finalize): round_epilogue
    RC_QUEUE = 16,      // + i, i < 8: the tile queue (common.h) of the call's colour launch
    RC_CLEARED = 24,    // counters cleared per call
    RC_RESERVED = 64    // ints the workspace holds
};
static_assert(RC_QUEUE + TQ_HEADS <= RC_CLEARED && RC_CLEARED <= RC_RESERVED && RC_CLEARED <= 256, "k_ray_coarse clears the counters with one 256-thread workgroup");

// coarse samples: z = near + (far-near) * linspace(0,1,S)  and their points, point index p = s*R + r
// t_rand (optional): the reference's stratified jitter (sparse_neus_renderer.py:506-515).  The reference draws
// t_rand = torch.rand(z_vals.shape) on the HOST ([R][S], ray-major) and sets z = lower + (upper - lower) * t_rand with
// lower/upper the midpoints to the neighbouring coarse samples; the caller hands the same tensor over, so the path is
// bit-reproducible under torch.manual_seed.  msk (optional, [S][R] bytes): 1 where the sample point lies in an occupied voxel of the mask volume
// (what up_sample asks of every sample, :84-88) -- kept next to z / sdf from here on, so that no later kernel has to gather it again.
__global__ __launch_bounds__(256) void k_ray_coarse(RayGeom g, float near, float far, const float* __restrict__ near_ray,
                                                    const float* __restrict__ far_ray, int S, const float* __restrict__ t_rand,
                                                    float* __restrict__ z, float* __restrict__ pts, const float* __restrict__ maskvol, int D,
                                                    uint8_t* __restrict__ msk, int* __restrict__ counters) {
    // o2345_render_rays: the first kernel of the call also clears the call's device-side counters (they are first touched by a later launch)
    if (counters && blockIdx.x == 0 && threadIdx.x < RC_CLEARED) counters[threadIdx.x] = 0;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long)S * g.R) return;
    const int s = (int)(p / g.R), r = (int)(p % g.R);
    if (near_ray) { near = near_ray[r]; far = far_ray[r]; }      // the reference's [N_rays, 1] near / far (:486-490): the same expression per ray
    float zz = near + (far - near) * linspace_at(0.f, 1.f, S, s);
    if (t_rand) {
        const float zp = near + (far - near) * linspace_at(0.f, 1.f, S, s > 0 ? s - 1 : 0);
        const float zn = near + (far - near) * linspace_at(0.f, 1.f, S, s < S - 1 ? s + 1 : S - 1);
        const float lower = s > 0 ? 0.5f * (zz + zp) : zz;            // mids = .5 * (z[1:] + z[:-1])
        const float upper = s < S - 1 ? 0.5f * (zn + zz) : zz;
        zz = lower + (upper - lower) * t_rand[(long long)r * S + s];
    }
    z[p] = zz;
    float x, y, w;
    ray_point(g, r, zz, x, y, w);
    pts[3 * p] = x; pts[3 * p + 1] = y; pts[3 * p + 2] = w;
    if (msk) msk[p] = mask_at(maskvol, D, x, y, w) > 0.f ? 1 : 0;
}

// Occupied points are appended to a global list (order inside the list is irrelevant for the results: they are scattered back by slot).  A wave
// reserves its range with ONE atomic by lane 0 (reserve_slots) and its lanes take their places by ballot + popcount prefix: no block barrier.
__device__ __forceinline__ unsigned long long lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }
// lane 0 of a wave: n list entries, counted for the rays' segment as well (segment mode).  All rays of a wave lie in ONE segment (seg_rays is a
// multiple of 64): that of ray0, any live ray of the wave.
__device__ __forceinline__ int reserve_slots(int* __restrict__ count, int n, int* __restrict__ seg_cnt, int ray0, int seg_rays) {
    const int base = atomicAdd(count, n);
    if (seg_cnt) atomicAdd(seg_cnt + ray0 / seg_rays, n);
    return base;
}
// "this lane has a slot to append" (the sixteen-lanes-per-ray kernels: one call per step of 64 (sample, ray) pairs)
__device__ __forceinline__ void append_lane(bool valid, int slot, int* __restrict__ list, int* __restrict__ count, int* __restrict__ seg_cnt = nullptr,
                                            int ray0 = 0, int seg_rays = 0) {
    const unsigned long long m = __ballot(valid);
    if (!m) return;
    int base = 0;
    if ((threadIdx.x & 63) == 0) base = reserve_slots(count, __popcll(m), seg_cnt, ray0, seg_rays);
    base = __shfl(base, 0);
    if (valid) list[base + __popcll(m & lanes_below())] = slot;
}
// One lane owns one ray and walks its samples (the streaming kernels): the wave first collects the validity of all (sample, ray) pairs it owns as
// bit masks, reserves its whole range at once, and then writes its slots sample by sample: 1/S of the atomics of a per-sample reservation.
struct ValidBits {                                   // up to 256 samples per ray
    unsigned w[8];
    __device__ __forceinline__ void set(int s) { w[s >> 5] |= 1u << (s & 31); }
    __device__ __forceinline__ bool get(int s) const { return (w[s >> 5] >> (s & 31)) & 1u; }
};
__device__ __forceinline__ void append_wave(const ValidBits& bits, int n_samples, int my_count, int R, int r,
                                            int* __restrict__ list, int* __restrict__ count, int* __restrict__ seg_cnt = nullptr, int seg_rays = 0) {
    int total = my_count;
#pragma unroll
    for (int off = 32; off; off >>= 1) total += __shfl_xor(total, off);
    int base = 0;
    if ((threadIdx.x & 63) == 0 && total) base = reserve_slots(count, total, seg_cnt, r, seg_rays);      // lane 0's ray is live when total > 0
    base = __shfl(base, 0);
    if (!total) return;
    const unsigned long long lt = lanes_below();
    for (int s = 0; s < n_samples; ++s) {
        const bool valid = bits.get(s);
        const unsigned long long m = __ballot(valid);
        if (valid) list[base + __popcll(m & lt)] = s * R + r;
        base += __popcll(m);
    }
}

// cat_z_vals quirk (:137): the SDF of the new points is evaluated only if MORE THAN ONE of them is inside the mask
// (o2345_render_rays applies it inside the round kernel: round_epilogue; this launch follows the stage entry o2345_ray_upsample)
__global__ void k_quirk_min2(int* count) { if (*count <= 1) *count = 0; }

// ---- one round of the hierarchical sampler (up_sample + sample_pdf, preceded by the cat_z_vals of the previous round; or that merge + render_core's head)
// A round is ONE kernel.  Three kernels per round (up-sample, merge, and the SDF network between them) that walk a ray's samples straight from the
// sample-major global lists, one lane per ray, make every step of the serial chains (transmittance, CDF walk, back-to-front merge) a DEPENDENT trip to
// L2 / HBM, 60 - 110 of them per ray and launch: measured 2.9 ms per 262,144 rays, and 81 / 40 / 95 us per launch for one 512-ray chunk of the
// reference's val loop.  Instead:
//   * cat_z_vals of the PREVIOUS round (its 16 new samples, now with their SDF values) is fused into the next kernel as a rank merge, and the last
//     merge into render_core's head (mid points, section lengths, occupancy, defaults, occupied-point list): four launches and two passes over the lists less;
//   * the occupancy flag of every sample point travels with the list (one byte per sample, written where the point is produced) instead of being
//     gathered from the mask volume again in every round;
//   * two forms of the same round, selected by the batch size (use_group_form), built from the same functions (render_math.h and the per-sample stages
//     below) and bit-identical to each other: k_ray_stream (large batches: one lane per ray, static access pattern, blocks of 8 rows in flight, full
//     occupancy -> HBM-bound) and k_ray_group (small batches: sixteen lanes per ray, only the two scans serial).
constexpr int NFIX = 16;                             // new samples per round held in registers (n_importance / 4 of the released configuration)
constexpr int RM_UPSAMPLE = 0, RM_FINALIZE = 1, RM_MERGE_ONLY = 2;

struct RoundArgs {
    RayGeom g;
    float* z; float* sdf; uint8_t* msk;              // the lists [rows][R] (msk may be null: occupancy is then gathered while staging)
    int S;                                           // samples per ray in the lists (before the merge)
    const float* new_z; const float* new_sdf; const uint8_t* new_msk; int n_new;      // previous round's samples to merge first (n_new = 0: none)
    const float* maskvol; int D;
    // upsample
    float inv_s; int n_imp;
    float* out_z; float* out_pts; float* out_sdf; uint8_t* out_msk; int* list; int* count;
    int* done;                                       // optional zeroed counter: the round applies the reference's per-call quirk itself (round_epilogue)
    // finalize
    float sample_dist;
    float* mid_z; float* dists; float* pts; float* pm; float* o_sdf; float* grad; float* rgb; int defaults_everywhere;
    int merge_all_lists;                             // finalize + merge: also read the new samples' sdf / occupancy and write the merged lists back.  Set nowhere:
                                                     // nobody reads them after the last round, and o2345_render_rays does not evaluate that SDF (it holds the default 100)
    // O2345RenderIO.segment_rays: the rays are consecutive render() calls of seg_rays rays evaluated together; the two per-call rules per segment
    int seg_rays, n_seg;                             // 0: the launch is one call
    int* seg_cnt;                                    // [n_seg] zeroed: list entries this round appends, per segment
    const int* seg_prev;                             // [n_seg] the PREVIOUS up-sampling round's counts: its new samples keep sdf = 100 where <= 1 (cat_z_vals :137)
};
// cat_z_vals' rule in segment mode: the SDF kernel has evaluated every listed new sample (at most ONE too many per segment); the merge that consumes
// them reads 100 instead wherever the sample's segment had at most one new sample inside the mask -- the value the reference leaves there.
__device__ __forceinline__ bool seg_keeps_default(const int* __restrict__ seg_prev, int seg_rays, int r) { return seg_prev && seg_prev[r / seg_rays] <= 1; }

// The reference's two per-CALL rules on the emitted list, applied by the round kernel itself instead of a one-thread launch each (six launches of the
// 22 of a 512-ray chunk): the workgroup that finishes LAST (a.done counts finished workgroups) sees the final count and
//   up-sampling round  cat_z_vals (:137): the SDF of the new samples is evaluated only if MORE THAN ONE of them is inside the mask -> count <= 1 becomes 0;
//   finalize           render_core (:222-223): with no occupied point at all the first 100 points of the chunk (ray 0, samples 0..99, in the
//                      reference's ray-major order) are evaluated anyway.
// Without a.done (the stage entry points) the launches k_quirk_min2 / nothing follow as before.
// Ordering without fences: `count` and `done` are only ever touched by agent-scope atomic read-modify-writes, which are performed at the device's
// coherent point; a workgroup's appends have RETURNED (their result is consumed) before its barrier, its increment of `done` is issued after the barrier,
// and the last workgroup reads `count` (an atomic again) after its own increment has returned -- so every append precedes that read.  An agent-scope
// fence (__threadfence) here is an L2 write-back of everything the kernel has written on this multi-XCD part: measured + 31 / 40 / 72 us per launch
// at 262,144 rays (profiles/NOTES.md), for an ordering the atomics already have.
template <int MODE>
__device__ __forceinline__ void round_epilogue(const RoundArgs& a, int S) {
    if (!a.done || MODE == RM_MERGE_ONLY) return;    // kernel argument: uniform over the launch
    if (a.seg_rays && MODE == RM_UPSAMPLE) return;   // segment mode: the merge that consumes the samples applies the rule (seg_keeps_default)
    __shared__ int last;
    __syncthreads();                                 // every append of this workgroup has returned its base
    if (threadIdx.x == 0) last = atomicAdd(a.done, 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    // (the reference sets pts_mask_bool[:100] on the RAY-MAJOR flattened [N_rays * S] mask: point t is (ray t / S, sample t % S) -- with S < 100 the rule
    //  runs on into the next rays; slots here are sample-major, s * R + r)
    if (a.seg_rays) {                                // render_core's rule per segment: a segment without any occupied point evaluates its first 100 points
        for (int k = threadIdx.x; k < a.n_seg; k += blockDim.x) {
            if (atomicAdd(a.seg_cnt + k, 0) >= 1) continue;
            const int r0 = k * a.seg_rays;
            const int rays = (a.g.R - r0) < a.seg_rays ? (a.g.R - r0) : a.seg_rays;
            const long long avail = (long long)rays * S;
            const int n = avail < 100 ? (int)avail : 100;
            const int base = atomicAdd(a.count, n);
            for (int t = 0; t < n; ++t) a.list[base + t] = (t % S) * a.g.R + r0 + t / S;
            atomicExch(a.seg_cnt + k, n);             // the segment's "evaluated points" (scalars[3])
        }
        return;
    }
    const int c = atomicAdd(a.count, 0);
    if (MODE == RM_UPSAMPLE) {
        if (threadIdx.x == 0 && c <= 1) atomicExch(a.count, 0);
    } else if (c < 1) {
        const long long avail = (long long)a.g.R * S;
        const int n = avail < 100 ? (int)avail : 100;
        for (int t = threadIdx.x; t < n; t += blockDim.x) a.list[t] = (t % S) * a.g.R + t / S;     // slot of (ray t / S, sample t % S)
        if (threadIdx.x == 0) atomicExch(a.count, n);
    }
}

// ---- the per-sample stages of a round, written once for both kernel forms --------------------------------------------------------------------
// Values in, stores out: the callers keep their loops, and the streaming kernel its blocks of 8 rows loaded before any of them is used.
struct NewSample { float z, sdf; unsigned tag; };   // one sample of the previous round's block as the merge takes it (tag: its occupancy flag)
template <int MODE>
__device__ __forceinline__ NewSample load_new_sample(const RoundArgs& a, int j, int rr, bool keeps_default) {
    const bool z_only = MODE == RM_FINALIZE && !a.merge_all_lists;      // the LAST cat_z_vals of a call: only the depths are read again (GlobalMergeZ)
    const size_t p = (size_t)j * a.g.R + rr;
    NewSample n;
    n.z = a.new_z[p];
    n.sdf = z_only ? 0.f : a.new_sdf[p];
    n.tag = (a.new_msk && !z_only) ? a.new_msk[p] : 0u;
    if (!z_only && keeps_default) n.sdf = 100.f;                        // seg_keeps_default
    if (MODE == RM_UPSAMPLE && !a.new_msk) n.tag = point_in_mask(a.g, rr, n.z, a.maskvol, a.D) ? 1u : 0u;      // no byte list came along: up_sample asks the volume
    return n;
}

// One new sample of an up-sampling round: its point, cat_z_vals' default SDF outside the mask (:135), its occupancy byte.  -> inside the mask
__device__ __forceinline__ bool emit_new_sample(const RoundArgs& a, size_t slot, float x, float y, float w, float m) {
    a.out_pts[3 * slot] = x; a.out_pts[3 * slot + 1] = y; a.out_pts[3 * slot + 2] = w;
    a.out_sdf[slot] = 100.f;
    const bool in = m > 0.f;
    if (a.out_msk) a.out_msk[slot] = in ? 1 : 0;
    return in;
}

// One sample of render_core's head (:204-231): section length (the last section: sample_dist), mid depth, mid point and its occupancy ...
struct MidSample { float d, z, x, y, w, m; };
__device__ __forceinline__ MidSample mid_sample(const RoundArgs& a, int rr, float zc, float z_next, bool last) {
    MidSample q;
    q.d = last ? a.sample_dist : z_next - zc;
    q.z = zc + q.d * 0.5f;
    ray_point(a.g, rr, q.z, q.x, q.y, q.w);
    q.m = mask_at(a.maskvol, a.D, q.x, q.y, q.w);
    return q;
}
// ... and its stores.  -> occupied.  The reference's defaults (:231: sdf = 100, gradients = colours = 0): inside o2345_render_rays occupied points are
// ALWAYS overwritten by the network kernels that consume the list (every list entry is evaluated), so only unoccupied points need them there: 28 bytes
// less per occupied point.  The public stage entry initialises every slot (defaults_everywhere: a caller may evaluate only part of the list).
__device__ __forceinline__ bool store_mid_sample(const RoundArgs& a, size_t p, const MidSample& q) {
    a.dists[p] = q.d; a.mid_z[p] = q.z; a.pm[p] = q.m;
    a.pts[3 * p] = q.x; a.pts[3 * p + 1] = q.y; a.pts[3 * p + 2] = q.w;
    const bool occ = q.m > 0.f;
    if (!occ || a.defaults_everywhere) {
        a.o_sdf[p] = 100.f;
        a.grad[3 * p] = 0.f; a.grad[3 * p + 1] = 0.f; a.grad[3 * p + 2] = 0.f;
        a.rgb[3 * p] = 0.f; a.rgb[3 * p + 1] = 0.f; a.rgb[3 * p + 2] = 0.f;
    }
    return occ;
}

// ---- the round as a STREAMING kernel: one lane per ray, the lists read from global memory ----------------------------------------------------
// Nothing is staged (an LDS-staged form -- 64 rays x 128 rows x 9 bytes per wave -- was measured: two waves per CU, 0.82 ms per round at
// 262,144 rays against 0.36 here): render_math.h's passes touch the lists at static, ascending rows in blocks of 8, so every block is one trip with 24
// loads in flight, eight waves per SIMD hide those trips, and a round is bound by its HBM traffic.  The section weights go through a global scratch
// row set (wbuf); in-place rank merge on the global lists (writes of a block of rows never reach a row not yet read).
struct GlobalMergeZ {                               // the LAST cat_z_vals of a render call: only the depths are read again (render_core re-evaluates the SDF at the mid points)
    float* z_; size_t R; int r;
    __device__ __forceinline__ float z(int i) const { return z_[(size_t)i * R + r]; }
    __device__ __forceinline__ float sdf(int) const { return 0.f; }
    __device__ __forceinline__ unsigned tag(int) const { return 0u; }
    __device__ __forceinline__ void put(int i, float zv, float, unsigned) { z_[(size_t)i * R + r] = zv; }
};

template <int MODE, bool MERGE>
__global__ __launch_bounds__(256) void k_ray_stream(RoundArgs a, float* __restrict__ wbuf) {
    const int R = a.g.R;
    const int r = blockIdx.x * 256 + threadIdx.x;
    const bool live = r < R;
    const int rr = live ? r : R - 1;
    int S = a.S;
    if (MERGE) {
        float nz[NFIX], ns[NFIX];
        unsigned nt[NFIX];
        const bool keeps_default = seg_keeps_default(a.seg_prev, a.seg_rays, rr);
#pragma unroll
        for (int j = 0; j < NFIX; ++j) {
            const NewSample n = load_new_sample<MODE>(a, j, rr, keeps_default);
            nz[j] = n.z; ns[j] = n.sdf; nt[j] = n.tag;
        }
        bool sorted = true;
#pragma unroll
        for (int j = 0; j + 1 < NFIX; ++j) sorted = sorted && !(nz[j] > nz[j + 1]);
        if (live) {                                 // in-place on the global lists: lanes past the last ray must not write
            if (MODE == RM_FINALIZE && !a.merge_all_lists) {
                GlobalMergeZ m{a.z, (size_t)R, r};
                merge_core_fixed<GlobalMergeZ, NFIX>(m, S, nz, ns, nt, sorted);
            } else {
                GlobalMergeTag m{a.z, a.sdf, a.msk, (size_t)R, r};
                merge_core_fixed<GlobalMergeTag, NFIX>(m, S, nz, ns, nt, sorted);
            }
        }
        S += NFIX;
    }
    if (MODE == RM_UPSAMPLE) {
        if (live) {
            GlobalRay acc{a.z, a.sdf, a.msk, wbuf, a.out_z, (size_t)R, r, a.g, a.maskvol, a.D};
            upsample_core(acc, S, a.inv_s, a.n_imp);
        }
        ValidBits bits{};
        int cnt = 0;
        for (int t0 = 0; t0 < a.n_imp; t0 += 8) {
            float m8[8], z8[8], p8[8][3];
#pragma unroll
            for (int k = 0; k < 8; ++k) z8[k] = a.out_z[(size_t)(t0 + k < a.n_imp ? t0 + k : a.n_imp - 1) * R + rr];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                ray_point(a.g, rr, z8[k], p8[k][0], p8[k][1], p8[k][2]);
                m8[k] = mask_at(a.maskvol, a.D, p8[k][0], p8[k][1], p8[k][2]);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int t = t0 + k;
                if (live && t < a.n_imp && emit_new_sample(a, (size_t)t * R + r, p8[k][0], p8[k][1], p8[k][2], m8[k])) { bits.set(t); ++cnt; }
            }
        }
        append_wave(bits, a.n_imp, cnt, R, r, a.list, a.count, a.seg_cnt, a.seg_rays);
    } else if (MODE == RM_FINALIZE) {
        ValidBits bits{};
        int cnt = 0;
        float znext = a.z[rr];
        for (int s0 = 0; s0 < S; s0 += 8) {
            float zc8[9];
            MidSample q8[8];
            zc8[0] = znext;
#pragma unroll
            for (int k = 1; k <= 8; ++k) zc8[k] = a.z[(size_t)(s0 + k < S ? s0 + k : S - 1) * R + rr];
            znext = zc8[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) q8[k] = mid_sample(a, rr, zc8[k], zc8[k + 1], s0 + k + 1 >= S);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int s = s0 + k;
                if (live && s < S && store_mid_sample(a, (size_t)s * R + r, q8[k])) { bits.set(s); ++cnt; }
            }
        }
        append_wave(bits, S, cnt, R, r, a.list, a.count, a.seg_cnt, a.seg_rays);
    }
    round_epilogue<MODE>(a, S);
}

// ---- the same round for SMALL batches: sixteen lanes per ray ---------------------------------------------------------------------------------------
// A 512-ray chunk of the reference's val loop (trainer_generic.py:415-416) is 8 waves with one lane per ray: every kernel of the round is one wave's
// ~20 k dependent instructions long whatever the GPU could do in parallel (50 - 130 us per launch with one lane per ray, x 6 launches x 128 chunks per
// image).  Only TWO things in a round are inherently serial per ray: the running transmittance / weight sum (pass 1) and the running CDF (pass 2) --
// two scans of ~110 two-operation steps whose order is the reference's order and is kept.  Everything else is element-wise per section / per sample and
// is spread over the 16 lanes of the ray's group (4 rays per wave, the lists of the 4 rays in LDS, ray-contiguous so that lane l reads row l + 16 i):
//   merge   rank merge: each existing sample finds #new < it (16 compares against the new block), each new sample its rank in the block and #old <= it
//           (binary search); out of place, in LDS;
//   pass 1  alpha_s of every section in parallel (upsample_section_alpha; a section recomputes its predecessor's slope) -> lane 0 runs the T / w / sum scan;
//   pass 2  pdf = w / sum in parallel -> lane 0 accumulates the CDF in order -> every new sample t does its own searchsorted (binary search) and
//           interpolation: identical to the forward walk, which stops at the first k with cdf_k > u_t as well;
//   points, occupancy and the list of the new samples in parallel (one ballot per wave).
// Same functions per element (render_math.h and the stages above), same order in the two scans => bit-identical to the streaming form
// (tests/test_gpu_parity.py).
constexpr int GL = 16, GR = 4;                       // lanes per ray, rays per wave
struct GroupRay {                                    // the lane's place in its 64-lane workgroup: lane l of the group of ray r
    int lane, sub, l, r, rr;                         // rr: r, or the last ray for the lanes past it (they compute, but do not write)
    bool live;
    __device__ __forceinline__ explicit GroupRay(int R)
        : lane(threadIdx.x), sub(lane >> 4), l(lane & 15), r(blockIdx.x * GR + sub), rr(r < R ? r : R - 1), live(r < R) {}
    // array k of this ray in the workgroup's LDS block [arrays][GR][cap]
    __device__ __forceinline__ float* row(float* lds, int k, int cap) const { return lds + (size_t)(k * GR + sub) * cap; }
};
// LDS arrays per ray of the three sixteen-lane kernels (kernel and launcher)
constexpr int GROUP_ARRAYS = 5, COMP_ARRAYS = 9, CULL_ARRAYS = 3;
__host__ __device__ constexpr size_t group_lds_bytes(int arrays, int cap) { return (size_t)arrays * GR * cap * sizeof(float); }
__host__ __device__ constexpr int round_cap(int rows) { return rows + 1; }       // k_ray_group: rows of the merged lists + 1

template <int MODE, bool MERGE>
__global__ __launch_bounds__(64) void k_ray_group(RoundArgs a) {
    extern __shared__ float lds[];
    const int R = a.g.R;
    const GroupRay q(R);
    const int l = q.l, r = q.r, rr = q.rr;
    int S = a.S;
    const int cap = round_cap(S + (MERGE ? NFIX : 0));
    float* zM = q.row(lds, 0, cap);                  // the (merged) lists of this ray
    float* sM = q.row(lds, 1, cap);
    float* mM = q.row(lds, 2, cap);
    float* xA = q.row(lds, 3, cap);                  // new block (merge) -> alpha -> w -> pdf
    float* cA = q.row(lds, 4, cap);                  // old depths (merge) -> cdf
    const bool need_mask = MODE == RM_UPSAMPLE;
    auto mask_of = [&](float zs) { return point_in_mask(a.g, rr, zs, a.maskvol, a.D) ? 1.f : 0.f; };
    if (!MERGE) {
        for (int i = l; i < S; i += GL) {
            const float zi = a.z[(size_t)i * R + rr];
            zM[i] = zi;
            sM[i] = a.sdf[(size_t)i * R + rr];
            if (need_mask) mM[i] = a.msk ? (float)a.msk[(size_t)i * R + rr] : mask_of(zi);
        }
        __syncthreads();
    } else {
        const NewSample nj = load_new_sample<MODE>(a, l, rr, seg_keeps_default(a.seg_prev, a.seg_rays, rr));      // lane j holds new sample j
        const float nzj = nj.z;
        xA[l] = nzj;
        for (int i = l; i < S; i += GL) cA[i] = a.z[(size_t)i * R + rr];
        __syncthreads();
        float nzv[NFIX];
#pragma unroll
        for (int k = 0; k < NFIX; ++k) nzv[k] = xA[k];
        int rank = 0;
#pragma unroll
        for (int k = 0; k < NFIX; ++k) rank += (nzv[k] < nzj || (nzv[k] == nzj && k < l)) ? 1 : 0;
        int lo = 0, hi = S;                                     // #old <= nzj (the old list is sorted)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cA[mid] <= nzj) lo = mid + 1; else hi = mid;
        }
        zM[rank + lo] = nzj; sM[rank + lo] = nj.sdf; mM[rank + lo] = (float)nj.tag;
        for (int i = l; i < S; i += GL) {
            const float zi = cA[i];
            int c = 0;
#pragma unroll
            for (int k = 0; k < NFIX; ++k) c += nzv[k] < zi ? 1 : 0;
            zM[i + c] = zi;
            sM[i + c] = a.sdf[(size_t)i * R + rr];
            if (need_mask || a.msk) mM[i + c] = a.msk ? (float)a.msk[(size_t)i * R + rr] : mask_of(zi);
        }
        __syncthreads();
        S += NFIX;
        if (q.live) {
            const bool z_only = MODE == RM_FINALIZE && !a.merge_all_lists;
            for (int i = l; i < S; i += GL) {
                a.z[(size_t)i * R + r] = zM[i];
                if (!z_only) {
                    a.sdf[(size_t)i * R + r] = sM[i];
                    if (a.msk) a.msk[(size_t)i * R + r] = (uint8_t)mM[i];
                }
            }
        }
    }
    if (MODE == RM_UPSAMPLE) {
        // pass 1: section opacities in parallel, then the transmittance / weight scan in the reference's order
        for (int sct = l; sct + 1 < S; sct += GL) {
            const float z0 = zM[sct], s0 = sM[sct], z1 = zM[sct + 1], s1 = sM[sct + 1];
            const float prev_dot = sct > 0 ? (s0 - sM[sct - 1]) / (z0 - zM[sct - 1] + 1e-5f) : 0.f;      // the previous section's dot_raw, recomputed
            float dot_raw;
            xA[sct] = upsample_section_alpha(z0, s0, mM[sct], z1, s1, mM[sct + 1], prev_dot, a.inv_s, dot_raw);
        }
        __syncthreads();
        float wsum = 0.f;
        if (l == 0) {
            float T = 1.f;
            for (int sct = 0; sct + 1 < S; ++sct) {
                const float w = transmit_step(T, xA[sct]) + 1e-5f;
                xA[sct] = w;
                wsum += w;
            }
        }
        wsum = __shfl(wsum, q.sub * GL);
        __syncthreads();
        // pass 2: pdf in parallel, CDF in order, then every new sample searches for itself
        for (int k = l; k + 1 < S; k += GL) xA[k] = xA[k] / wsum;
        __syncthreads();
        if (l == 0) {
            float c = 0.f;
            cA[0] = 0.f;
            for (int k = 1; k < S; ++k) { c = c + xA[k - 1]; cA[k] = c; }
        }
        __syncthreads();
        for (int t0 = 0; t0 < a.n_imp; t0 += GL) {
            const int t = t0 + l;
            bool in = false;
            if (t < a.n_imp) {
                const float u = upsample_u(a.n_imp, t);
                int lo = 0, hi = S;                                 // searchsorted(right = True): first k with cdf[k] > u (k >= 1 since cdf[0] = 0 < u), else S
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (cA[mid] > u) hi = mid; else lo = mid + 1;
                }
                const int k = lo;
                const float cb = cA[k - 1];
                const float zn = inverse_cdf_z(u, cb, k == S ? cb : cA[k], k == S, zM[k - 1], zM[k < S ? k : S - 1]);
                float x, y, w;
                ray_point(a.g, rr, zn, x, y, w);
                const float m = mask_at(a.maskvol, a.D, x, y, w);
                if (q.live) {
                    const size_t slot = (size_t)t * R + r;
                    a.out_z[slot] = zn;
                    in = emit_new_sample(a, slot, x, y, w, m);
                }
            }
            append_lane(in, t * R + r, a.list, a.count, a.seg_cnt, blockIdx.x * GR, a.seg_rays);
        }
    } else if (MODE == RM_FINALIZE) {
        for (int s0 = 0; s0 < S; s0 += GL) {
            const int smp = s0 + l;
            bool occ = false;
            if (smp < S && q.live) {
                const bool last = smp + 1 >= S;
                occ = store_mid_sample(a, (size_t)smp * R + r, mid_sample(a, r, zM[smp], last ? 0.f : zM[smp + 1], last));
            }
            append_lane(occ, smp * R + r, a.list, a.count, a.seg_cnt, blockIdx.x * GR, a.seg_rays);
        }
    }
    round_epilogue<MODE>(a, S);
}

// cat_z_vals for a block size other than NFIX: the plain per-ray merge on the global lists (render_math.h merge_core), occupancy bytes along
__global__ __launch_bounds__(64) void k_ray_merge_any(int R, float* z, float* sdf, uint8_t* msk, int S, const float* new_z, const float* new_sdf,
                                                      const uint8_t* new_msk, int n_new, const int* seg_prev, int seg_rays) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    const bool keep_default = seg_keeps_default(seg_prev, seg_rays, r);
    constexpr int NMAX = 32;
    float nz[NMAX], ns[NMAX];
    unsigned nt[NMAX];
    for (int base = 0; base < n_new; base += NMAX) {
        const int nb = n_new - base < NMAX ? n_new - base : NMAX;
        for (int j = 0; j < nb; ++j) {
            nz[j] = new_z[(size_t)(base + j) * R + r]; ns[j] = keep_default ? 100.f : new_sdf[(size_t)(base + j) * R + r];
            nt[j] = new_msk ? new_msk[(size_t)(base + j) * R + r] : 0u;
        }
        GlobalMergeTag a{z, sdf, msk, (size_t)R, r};
        ArrayBlock blk{nz, ns, nt};
        merge_core(a, S + base, blk, nb);
    }
}

// ---- render_core's compositing ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_ray_composite(RayGeom g, int S, const float* __restrict__ mid_z, const float* __restrict__ dists,
                                                       const float* __restrict__ pm, const float* __restrict__ sdf,
                                                       const float* __restrict__ grad, const float* __restrict__ rgb,
                                                       const uint8_t* __restrict__ nviews, float inv_s, float air, float bg,
                                                       CompositeOut o) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r < g.R) composite_ray(g, r, S, mid_z, dists, pm, sdf, grad, rgb, nviews, inv_s, air, bg, o);
}

// The same for small batches, sixteen lanes per ray: per-sample opacities and products in parallel, ONE lane runs the ordered accumulation
// (composite_ray's own CompositeSums) out of LDS, the per-sample outputs are written in parallel.
__global__ __launch_bounds__(64) void k_ray_composite_group(RayGeom g, int S, const float* __restrict__ mid_z, const float* __restrict__ dists,
                                                            const float* __restrict__ pm, const float* __restrict__ sdf,
                                                            const float* __restrict__ grad, const float* __restrict__ rgb,
                                                            const uint8_t* __restrict__ nviews, float inv_s, float air, float bg, CompositeOut o) {
    extern __shared__ float lds[];
    const int R = g.R;
    const GroupRay q(R);
    const int l = q.l, r = q.r, rr = q.rr;
    float* L[COMP_ARRAYS];
#pragma unroll
    for (int k = 0; k < COMP_ARRAYS; ++k) L[k] = q.row(lds, k, S);
    float *aL = L[0], *c0L = L[1], *c1L = L[2], *c2L = L[3], *zL = L[4], *gL = L[5], *mL = L[6], *nL = L[7], *wL = L[8];
    const float dx = g.rays_d[3 * rr], dy = g.rays_d[3 * rr + 1], dz = g.rays_d[3 * rr + 2];
    for (int smp = l; smp < S; smp += GL) {
        const size_t p = (size_t)smp * R + rr;
        const float m = pm[p];
        const float gx = grad[3 * p], gy = grad[3 * p + 1], gz = grad[3 * p + 2];
        float pc;
        aL[smp] = composite_sample_alpha(dx, dy, dz, gx, gy, gz, m, dists[p], sdf[p], inv_s, air, pc);
        if (q.live) o.cdf[p] = pc;
        c0L[smp] = rgb[3 * p]; c1L[smp] = rgb[3 * p + 1]; c2L[smp] = rgb[3 * p + 2];
        zL[smp] = mid_z[p];
        gL[smp] = gradient_error(gx, gy, gz, m);
        mL[smp] = m;
        nL[smp] = nviews[p] >= 2 ? 1.f : 0.f;
    }
    __syncthreads();
    if (l == 0 && q.live) {
        CompositeSums sum;
        for (int smp = 0; smp < S; ++smp) wL[smp] = sum.add(aL[smp], c0L[smp], c1L[smp], c2L[smp], zL[smp], gL[smp], mL[smp], nL[smp] > 0.f);
        sum.finish(o, r, bg);
        for (int smp = 0; smp < S; ++smp) sum.add_var(zL[smp], wL[smp]);
        sum.finish_var(o, r);
    }
    __syncthreads();
    if (q.live)
        for (int smp = l; smp < S; smp += GL) o.weights[(size_t)smp * R + r] = wL[smp];
}

// ---- tolerance-bounded colour work removal (O2345RenderIO.weight_cull) ------------------------------------------------------------------------
// After the SDF + gradient pass every compositing weight w = alpha * T is known -- it does not depend on the colours.  This pass runs composite_ray's
// transmittance chain (the SAME functions in the same order: the w it thresholds is bit-identical to the `weights` the composite kernel returns) and
// emits the list of the occupied samples with w >= thr: only those go through the visibility sort and the colour network.  keep[p] = 1 there, 0 on
// every other slot (unoccupied or culled: the counting kernel supplies their valid-view counts, so the per-ray colour mask stays exact); culled occupied
// samples get the colour 0 the composite kernel will multiply by their w < thr.
// -> the sample stays in the list
__device__ __forceinline__ bool cull_sample(bool live, float m, float w, float thr, size_t p, float* __restrict__ keep, float* __restrict__ rgb) {
    const bool occ = m > 0.f;
    const bool kp = live && occ && w >= thr;
    if (live) {
        keep[p] = kp ? 1.f : 0.f;
        if (occ && !kp) { rgb[3 * p] = 0.f; rgb[3 * p + 1] = 0.f; rgb[3 * p + 2] = 0.f; }
    }
    return kp;
}

__global__ __launch_bounds__(256) void k_ray_cull(RayGeom g, int S, const float* __restrict__ dists, const float* __restrict__ pm, const float* __restrict__ sdf,
                                                  const float* __restrict__ grad, float inv_s, float air, float thr, float* __restrict__ keep,
                                                  float* __restrict__ rgb, int* __restrict__ list, int* __restrict__ count) {
    const int R = g.R;
    const int r = blockIdx.x * 256 + threadIdx.x;
    const bool live = r < R;
    const int rr = live ? r : R - 1;
    const float dx = g.rays_d[3 * rr], dy = g.rays_d[3 * rr + 1], dz = g.rays_d[3 * rr + 2];
    ValidBits bits{};
    int cnt = 0;
    float T = 1.f;
    constexpr int CB = 8;
    for (int sb = 0; sb < S; sb += CB) {
        float bm[CB], bd[CB], bs[CB], bg[CB][3];
#pragma unroll
        for (int k = 0; k < CB; ++k) {
            const int s = sb + k < S ? sb + k : S - 1;
            const size_t p = (size_t)s * R + rr;
            bm[k] = pm[p]; bd[k] = dists[p]; bs[k] = sdf[p];
            bg[k][0] = grad[3 * p]; bg[k][1] = grad[3 * p + 1]; bg[k][2] = grad[3 * p + 2];
        }
#pragma unroll
        for (int k = 0; k < CB; ++k) {
            if (sb + k < S) {
                const int s = sb + k;
                float pc;
                const float alpha = composite_sample_alpha(dx, dy, dz, bg[k][0], bg[k][1], bg[k][2], bm[k], bd[k], bs[k], inv_s, air, pc);
                const float w = transmit_step(T, alpha);
                if (cull_sample(live, bm[k], w, thr, (size_t)s * R + rr, keep, rgb)) { bits.set(s); ++cnt; }
            }
        }
    }
    append_wave(bits, S, cnt, R, rr, list, count);
}

// The same for SMALL batches, sixteen lanes per ray (cf. k_ray_composite_group): the per-sample opacities in parallel, ONE lane runs the transmittance scan in
// the reference's order, the threshold test and the list append in parallel again.  A 512-ray chunk: 62 us with one lane per ray (128 dependent steps of two
// exponentials and a division each), ~20 us here.  Same functions, same order in the scan: the same w, the same list (as a set), the same flags.
__global__ __launch_bounds__(64) void k_ray_cull_group(RayGeom g, int S, const float* __restrict__ dists, const float* __restrict__ pm, const float* __restrict__ sdf,
                                                       const float* __restrict__ grad, float inv_s, float air, float thr, float* __restrict__ keep,
                                                       float* __restrict__ rgb, int* __restrict__ list, int* __restrict__ count) {
    extern __shared__ float lds[];
    const int R = g.R;
    const GroupRay q(R);
    const int l = q.l, r = q.r, rr = q.rr;
    float* aL = q.row(lds, 0, S);
    float* mL = q.row(lds, 1, S);
    float* wL = q.row(lds, 2, S);
    const float dx = g.rays_d[3 * rr], dy = g.rays_d[3 * rr + 1], dz = g.rays_d[3 * rr + 2];
    for (int smp = l; smp < S; smp += GL) {
        const size_t p = (size_t)smp * R + rr;
        const float m = pm[p];
        float pc;
        aL[smp] = composite_sample_alpha(dx, dy, dz, grad[3 * p], grad[3 * p + 1], grad[3 * p + 2], m, dists[p], sdf[p], inv_s, air, pc);
        mL[smp] = m;
    }
    __syncthreads();
    if (l == 0) {
        float T = 1.f;
        for (int smp = 0; smp < S; ++smp) wL[smp] = transmit_step(T, aL[smp]);
    }
    __syncthreads();
    for (int s0 = 0; s0 < S; s0 += GL) {
        const int smp = s0 + l;
        const bool kp = smp < S && cull_sample(q.live, mL[smp], wL[smp], thr, (size_t)smp * R + rr, keep, rgb);
        append_lane(kp, smp * R + r, list, count);
    }
}

// per-call scalars of render()'s returned dict (:586-633): sums over the rays in a FIXED order (thread t adds rays t, t + 1024, ... in fp64, then a
// fixed LDS tree): deterministic, one workgroup, no atomics.  out[0] = alpha_sum.mean(), out[1] = alpha_sum.sum() / (R S) ("alpha_mean"),
// out[2] = sum grad_err[.,0] / (sum grad_err[.,1] + 1e-5) ("gradient_error_fine"), out[3] = number of list entries the network kernels evaluated.
// Segment mode (seg_rays > 0): workgroup k reduces the rays of segment k in the order a call on that segment alone would -> out[k][0..3].
__global__ __launch_bounds__(1024) void k_ray_scalars(int R_all, int S, const float* __restrict__ alpha_sum, const float* __restrict__ grad_err,
                                                      const int* __restrict__ count, float* __restrict__ out, int seg_rays) {
    __shared__ double red[3][1024];
    const int r0 = seg_rays ? (int)blockIdx.x * seg_rays : 0;
    const int R = seg_rays ? (R_all - r0 < seg_rays ? R_all - r0 : seg_rays) : R_all;
    alpha_sum += r0; grad_err += 2 * (size_t)r0; count += seg_rays ? blockIdx.x : 0; out += 4 * (size_t)blockIdx.x;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int r = threadIdx.x; r < R; r += 1024) { a += (double)alpha_sum[r]; b += (double)grad_err[2 * r]; c += (double)grad_err[2 * r + 1]; }
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = b; red[2][threadIdx.x] = c;
    __syncthreads();
    for (int off = 512; off; off >>= 1) {
        if ((int)threadIdx.x < off) {
            red[0][threadIdx.x] += red[0][threadIdx.x + off]; red[1][threadIdx.x] += red[1][threadIdx.x + off]; red[2][threadIdx.x] += red[2][threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (float)(red[0][0] / (double)R);
        out[1] = (float)(red[0][0] / ((double)R * (double)S));
        out[2] = (float)(red[1][0] / (red[2][0] + 1e-5));
        out[3] = (float)*count;
    }
}

// ---- host side: which kernel form, the round's instantiations, the workspace of a render call ------------------------------------------------
// Small batches take the sixteen-lanes-per-ray kernels (csrc/common.h knobs(): O2345_RAY_STREAM_MIN) where their lists fit the 64 KB of LDS a
// workgroup can have, everything else the streaming kernels.
static bool use_group_form(long long R, size_t lds_bytes) { return R < knobs().ray_stream_min && lds_bytes <= 64 * 1024; }

// The two families of round kernels, and the (mode, merge) instantiations either has
struct StreamRound {
    template <int MODE, bool MERGE> static void launch(const RoundArgs& a, float* wbuf, size_t, hipStream_t s) {
        hipLaunchKernelGGL((k_ray_stream<MODE, MERGE>), dim3(cdiv(a.g.R, 256)), dim3(256), 0, s, a, wbuf);
    }
};
struct GroupRound {
    template <int MODE, bool MERGE> static void launch(const RoundArgs& a, float*, size_t lds, hipStream_t s) {
        hipLaunchKernelGGL((k_ray_group<MODE, MERGE>), dim3(cdiv(a.g.R, GR)), dim3(64), lds, s, a);
    }
};
template <class FORM>
static void round_dispatch(int mode, bool merge, const RoundArgs& a, float* wbuf, size_t lds, hipStream_t s) {
    if (mode == RM_UPSAMPLE) merge ? FORM::template launch<RM_UPSAMPLE, true>(a, wbuf, lds, s) : FORM::template launch<RM_UPSAMPLE, false>(a, wbuf, lds, s);
    else if (mode == RM_FINALIZE) merge ? FORM::template launch<RM_FINALIZE, true>(a, wbuf, lds, s) : FORM::template launch<RM_FINALIZE, false>(a, wbuf, lds, s);
    else if (merge) FORM::template launch<RM_MERGE_ONLY, true>(a, wbuf, lds, s);
}

// The occupied-point list is grouped by view-visibility signature only where that pays: the sort is 4 launches per 8 views and costs 0.1 - 0.25 ms
// whatever the list length, the colour kernel gains ~10 % of its time.  Below 2^20 sample slots (a 512-ray chunk of the reference's val loop has
// 65,536: colour kernel 0.5 ms) the emission order is kept.  O2345_LIST_SORT=0 disables the sort everywhere (A/B knob).
static bool render_sorts_list(int R, int n_samples, int n_importance, int V) {
    return knobs().list_sort && V <= 32 && ((long long)n_samples + n_importance) * (long long)R >= (1ll << 20);
}

// The workspace of a render call: byte offset of every buffer, and the size of the whole.  S = n_samples + n_importance rows per ray in the end,
// NI = n_importance / 4 new samples per round, R rays; sample-major [rows][R].
struct RenderLayout {
    struct Span { size_t offset, bytes; };           // bytes = 0: the call does not have this buffer
    Span z, sdf, new_z, new_sdf, pts, list, counters, msk, new_msk, wbuf, cull_list, seg_counters, sorted_list, sort_ws;
    size_t total;
    template <class T> static T* at(void* workspace, const Span& b) { return b.bytes ? (T*)((char*)workspace + b.offset) : nullptr; }
};
static RenderLayout render_layout(int R_, int n_samples, int n_importance, int V) {
    const size_t R = (size_t)R_, S = (size_t)n_samples + n_importance, NI = (size_t)(n_importance / 4 > 0 ? n_importance / 4 : 1);
    const bool streams = (long long)R_ >= knobs().ray_stream_min, sorts = render_sorts_list(R_, n_samples, n_importance, V);
    size_t end = 0;
    auto take = [&end](size_t bytes, size_t align) {
        const size_t offset = (end + align - 1) / align * align;
        end = offset + bytes;
        return RenderLayout::Span{offset, bytes};
    };
    RenderLayout l;
    l.z = take(S * R * sizeof(float), 4);                            // the sorted sample lists: depth,
    l.sdf = take(S * R * sizeof(float), 4);                          //   SDF (dead after the last merge: then the keep flags of the weight cull),
    l.new_z = take(NI * R * sizeof(float), 4);                       // the round's new samples: depth,
    l.new_sdf = take(NI * R * sizeof(float), 4);                     //   SDF
    l.pts = take(3 * S * R * sizeof(float), 4);                      // points of the coarse / new / mid samples
    l.list = take(S * R * sizeof(int), 4);                           // occupied-point list of the round
    l.counters = take(RC_RESERVED * sizeof(int), 4);                 // RenderCounter
    l.msk = take(S * R, 1);                                          // occupancy byte of every listed sample,
    l.new_msk = take(NI * R, 1);                                     //   of the round's new samples
    l.wbuf = take(streams ? S * R * sizeof(float) : 0, 4);           // section weights (streaming up-sample kernel only)
    l.cull_list = take(S * R * sizeof(int), 256);                    // the weight-culled list (weight_cull > 0)
    l.seg_counters = take(5 * (R / 64 + 1) * sizeof(int), 256);      // [5 rounds][segments] list entries per segment (segment_rays > 0)
    l.sorted_list = take(sorts ? S * R * sizeof(int) : 0, 256);      // the list grouped by visibility (render_sorts_list),
    l.sort_ws = take(sorts ? o2345_list_sort_workspace_bytes((long long)(S * R), V) : 0, 4);      //   and the sort's own workspace (csrc/list_sort.hip)
    l.total = end;
    return l;
}

}  // namespace o2345

using namespace o2345;

extern "C" {

// ---- stage entry points (used by the parity tests; the orchestrator below calls the same kernels) -----------------
static int ray_coarse_launch(const float* rays_o, const float* rays_d, int R, float near, float far, const float* near_ray, const float* far_ray, int S,
                             const float* t_rand, float* z, float* pts, const float* maskvol, int D, uint8_t* msk, void* stream, int* counters = nullptr) {
    O2345_REQUIRE(rays_o && rays_d && z && pts && R > 0 && S > 1, "ray_coarse: bad arguments");
    O2345_REQUIRE((near_ray != nullptr) == (far_ray != nullptr), "ray_coarse: per-ray near and far come together");
    RayGeom g{rays_o, rays_d, R};
    hipLaunchKernelGGL(k_ray_coarse, dim3(cdiv((long long)R * S, 256)), dim3(256), 0, (hipStream_t)stream, g, near, far, near_ray, far_ray, S, t_rand, z, pts,
                       maskvol, D, msk, counters);
    return check_launch("ray_coarse");
}

int o2345_ray_coarse_jitter(const float* rays_o, const float* rays_d, int R, float near, float far, int S, const float* t_rand,
                            float* z, float* pts, void* stream) {
    return ray_coarse_launch(rays_o, rays_d, R, near, far, nullptr, nullptr, S, t_rand, z, pts, nullptr, 0, nullptr, stream);
}

int o2345_ray_coarse_per_ray(const float* rays_o, const float* rays_d, int R, const float* near_ray, const float* far_ray, int S,
                             const float* t_rand, float* z, float* pts, void* stream) {
    O2345_REQUIRE(near_ray && far_ray, "ray_coarse_per_ray: null pointer");
    return ray_coarse_launch(rays_o, rays_d, R, 0.f, 0.f, near_ray, far_ray, S, t_rand, z, pts, nullptr, 0, nullptr, stream);
}

int o2345_ray_coarse(const float* rays_o, const float* rays_d, int R, float near, float far, int S, float* z, float* pts, void* stream) {
    return o2345_ray_coarse_jitter(rays_o, rays_d, R, near, far, S, nullptr, z, pts, stream);
}

// One round launch.  A merge of exactly NFIX samples runs fused; any other block size is merged on the global lists first (k_ray_merge_any).
static int ray_round_launch(int mode, RoundArgs a, float* wbuf /* [rows][R] scratch of the streaming up-sample kernel, or null */, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int R = a.g.R;
    if (a.n_new > 0 && a.n_new != NFIX) {
        hipLaunchKernelGGL(k_ray_merge_any, dim3(cdiv(R, 64)), dim3(64), 0, s, R, a.z, a.sdf, a.msk, a.S, a.new_z, a.new_sdf, a.new_msk, a.n_new, a.seg_prev, a.seg_rays);
        a.seg_prev = nullptr;                    // applied
        a.S += a.n_new;
        a.n_new = 0;
        if (mode == RM_MERGE_ONLY) return check_launch("ray_merge");
    }
    const bool merge = a.n_new > 0;
    const int rows = a.S + (merge ? NFIX : 0);
    const size_t lds = group_lds_bytes(GROUP_ARRAYS, round_cap(rows));
    if (use_group_form(R, lds) || (mode == RM_UPSAMPLE && !wbuf)) {      // the streaming up-sample kernel needs its scratch rows
        O2345_REQUIRE(lds <= 64 * 1024, "ray kernels: %d list rows per ray (at most 600)", rows);
        round_dispatch<GroupRound>(mode, merge, a, nullptr, lds, s);
        return check_launch("ray_round");
    }
    round_dispatch<StreamRound>(mode, merge, a, wbuf, 0, s);
    return check_launch("ray_round (streaming)");
}

// ---- stage entry points (used by the parity tests; the orchestrator below launches the same kernel with the merge fused in) -----------------
int o2345_ray_upsample(const float* rays_o, const float* rays_d, int R, const float* z, const float* sdf, int S, float inv_s,
                       const float* maskvol, int D, float* wbuf, int n_imp, float* new_z, float* new_pts, float* new_sdf,
                       int32_t* list, int32_t* count_dev, void* stream) {
    O2345_REQUIRE(rays_o && rays_d && z && sdf && maskvol && new_z && new_pts && new_sdf && list && count_dev, "ray_upsample: null pointer");
    O2345_REQUIRE(n_imp >= 1 && n_imp <= 256 && S >= 2 && R > 0, "ray_upsample: 1..256 new samples per call, at least 2 samples per ray (got %d, %d)", n_imp, S);
    hipStream_t s = (hipStream_t)stream;
    O2345_HIP(hipMemsetAsync(count_dev, 0, sizeof(int), s));
    RoundArgs a{};
    a.g = RayGeom{rays_o, rays_d, R};
    a.z = const_cast<float*>(z); a.sdf = const_cast<float*>(sdf); a.S = S;          // read-only without a merge
    a.maskvol = maskvol; a.D = D; a.inv_s = inv_s; a.n_imp = n_imp;
    a.out_z = new_z; a.out_pts = new_pts; a.out_sdf = new_sdf; a.list = list; a.count = count_dev;
    int rc = ray_round_launch(RM_UPSAMPLE, a, wbuf, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_quirk_min2, dim3(1), dim3(1), 0, s, count_dev);
    return check_launch("ray_upsample");
}

int o2345_ray_merge(int R, float* z, float* sdf, int S, float* new_z, float* new_sdf, int n_new, void* stream) {
    O2345_REQUIRE(z && sdf && new_z && new_sdf && R > 0 && S >= 1 && n_new >= 1, "ray_merge: bad arguments");
    RoundArgs a{};
    a.g = RayGeom{nullptr, nullptr, R};
    a.z = z; a.sdf = sdf; a.S = S; a.new_z = new_z; a.new_sdf = new_sdf; a.n_new = n_new;
    return ray_round_launch(RM_MERGE_ONLY, a, nullptr, stream);
}

int o2345_ray_finalize(const float* rays_o, const float* rays_d, int R, const float* z, int S, float sample_dist,
                       const float* maskvol, int D, float* mid_z, float* dists, float* pts, float* pm, float* sdf,
                       float* grad, float* rgb, int32_t* list, int32_t* count_dev, void* stream) {
    O2345_REQUIRE(rays_o && rays_d && z && maskvol && mid_z && dists && pts && pm && sdf && grad && rgb && list && count_dev, "ray_finalize: null pointer");
    O2345_REQUIRE(S >= 1 && S <= 256 && R > 0, "ray_finalize: at most 256 samples per ray (got %d)", S);
    O2345_HIP(hipMemsetAsync(count_dev, 0, sizeof(int), (hipStream_t)stream));
    RoundArgs a{};
    a.g = RayGeom{rays_o, rays_d, R};
    a.z = const_cast<float*>(z); a.sdf = const_cast<float*>(z); a.S = S;            // the SDF list is not used by the finalize step (staged, never read)
    a.maskvol = maskvol; a.D = D; a.sample_dist = sample_dist;
    a.mid_z = mid_z; a.dists = dists; a.pts = pts; a.pm = pm; a.o_sdf = sdf; a.grad = grad; a.rgb = rgb; a.defaults_everywhere = 1;
    a.list = list; a.count = count_dev;
    return ray_round_launch(RM_FINALIZE, a, nullptr, stream);
}

int o2345_ray_composite(const float* rays_o, const float* rays_d, int R, int S, const float* mid_z, const float* dists,
                        const float* pm, const float* sdf, const float* grad, const float* rgb, const uint8_t* nviews,
                        float inv_s, float alpha_inter_ratio, float background, float* color, float* depth, float* weights,
                        float* cdf, float* weights_sum, float* weights_max, float* depth_var, float* alpha_sum,
                        float* grad_err, uint8_t* color_mask, void* stream) {
    O2345_REQUIRE(rays_o && rays_d && mid_z && dists && pm && sdf && grad && rgb && nviews && color && depth && weights && cdf &&
                  weights_sum && weights_max && depth_var && alpha_sum && grad_err && color_mask, "ray_composite: null pointer");
    RayGeom g{rays_o, rays_d, R};
    CompositeOut o{color, depth, weights, cdf, weights_sum, weights_max, depth_var, alpha_sum, grad_err, color_mask};
    const size_t lds = group_lds_bytes(COMP_ARRAYS, S);
    if (use_group_form(R, lds))
        hipLaunchKernelGGL(k_ray_composite_group, dim3(cdiv(R, GR)), dim3(64), lds, (hipStream_t)stream, g, S, mid_z, dists, pm, sdf, grad, rgb, nviews, inv_s,
                           alpha_inter_ratio, background, o);
    else
        hipLaunchKernelGGL(k_ray_composite, dim3(cdiv(R, 64)), dim3(64), 0, (hipStream_t)stream, g, S, mid_z, dists, pm, sdf, grad, rgb, nviews, inv_s, alpha_inter_ratio, background, o);
    return check_launch("ray_composite");
}

// ---- the whole render() call -----------------------------------------------------------------------------------------
size_t o2345_render_workspace_bytes(int R, int n_samples, int n_importance, int V) { return render_layout(R, n_samples, n_importance, V).total; }

int o2345_render_rays(const O2345RenderIO* io, void* workspace, size_t workspace_bytes, void* stream) {
    O2345_REQUIRE(io && workspace, "render_rays: null pointer");
    const int R = io->R, NS = io->n_samples, NIMP = io->n_importance;
    O2345_REQUIRE(NIMP % 4 == 0 && NIMP > 0 && NS > 1, "render_rays: n_importance must be a positive multiple of 4");
    O2345_REQUIRE(R > 0 && ((long long)NS + NIMP) * (long long)R < 2147483647LL, "render_rays: R * (n_samples + n_importance) must stay below 2^31 "
                  "(sample slots are 32-bit); split the ray batch (got R = %d)", R);
    const RenderLayout lay = render_layout(R, NS, NIMP, io->V);
    O2345_REQUIRE(workspace_bytes >= lay.total, "render_rays: workspace too small");
    O2345_REQUIRE(io->color_x3_blob || io->color_mfma_blob, "render_rays: a colour network blob is required (color_x3_blob or color_mfma_blob)");
    O2345_REQUIRE((io->near_ray != nullptr) == (io->far_ray != nullptr), "render_rays: per-ray near and far come together");
    const size_t S = (size_t)NS + NIMP, NI = NIMP / 4, RR = R;
    O2345_REQUIRE(S <= 256, "render_rays: at most 256 samples per ray (got %d)", (int)S);
    float* z = lay.at<float>(workspace, lay.z);
    float* sdf = lay.at<float>(workspace, lay.sdf);
    float* new_z = lay.at<float>(workspace, lay.new_z);
    float* new_sdf = lay.at<float>(workspace, lay.new_sdf);
    float* pts = lay.at<float>(workspace, lay.pts);
    int* list = lay.at<int>(workspace, lay.list);
    int* counters = lay.at<int>(workspace, lay.counters);
    uint8_t* msk = lay.at<uint8_t>(workspace, lay.msk);
    uint8_t* new_msk = lay.at<uint8_t>(workspace, lay.new_msk);
    float* wbuf = lay.at<float>(workspace, lay.wbuf);                 // null below ray_stream_min
    hipStream_t s = (hipStream_t)stream;
    int rc;
    O2345_REQUIRE(io->sdf_mode == 0 || io->sdf_mode == 2, "render_rays: SDF mode %d (0 = fp32, 2 = split-f16; the bf16 mode 1 was removed)", io->sdf_mode);
    // segment mode: the rays are consecutive render() calls of G rays each, evaluated together, the reference's two per-call rules applied per segment
    const int G = io->segment_rays;
    O2345_REQUIRE(G >= 0 && G % 64 == 0, "render_rays: segment_rays must be 0 or a multiple of 64 (got %d)", G);
    O2345_REQUIRE(G == 0 || !io->near_ray, "render_rays: segment_rays needs one near / far pair (sample_dist is a per-call mean for per-ray near / far)");
    const int n_seg = G ? (R + G - 1) / G : 0;
    int* segc = lay.at<int>(workspace, lay.seg_counters);                               // [5][n_seg]
    if (G) O2345_HIP(hipMemsetAsync(segc, 0, (size_t)5 * n_seg * sizeof(int), s));
    auto sdf_eval = [&](int variant, const float* p, const int* idx, const int* cnt, long long n, float* out, float* grad) {
        if (io->sdf_mode == 2 && variant == 0) return o2345_sdf_mlp_x3(io->sdf_blob, io->vol_cl, io->D, p, idx, cnt, n, 0, 1.f, out, stream);
        if (io->sdf_mode == 2 && variant == 2) return o2345_sdf_grad_x3(io->sdf_blob, io->vol_cl, io->D, p, idx, cnt, n, 0, 1.f, out, grad, stream);
        return o2345_sdf_mlp(variant, io->sdf_blob, io->vol_cl, io->D, p, idx, cnt, n, 0, 1.f, out, nullptr, nullptr, grad, stream);
    };
    // the first kernel also clears the call's counters
    if ((rc = ray_coarse_launch(io->rays_o, io->rays_d, R, io->near, io->far, io->near_ray, io->far_ray, NS, io->t_rand, z, pts, io->maskvol, io->D, msk, stream, counters))) return rc;
    // coarse SDF on ALL points (not masked, :525-528)
    if ((rc = sdf_eval(0, pts, nullptr, nullptr, (long long)NS * R, sdf, nullptr))) return rc;
    // four up-sampling rounds (:531-547); round i > 0 first merges round i - 1's samples (cat_z_vals) inside the same kernel.  The SDF of the new
    // samples is evaluated after rounds 0 - 2 only: round 3's samples are merged by the finalize round, which takes their depths alone (z_only in
    // load_new_sample), and render_core evaluates the SDF again at the mid points -- the reference deletes the SDF its last cat_z_vals returns unread
    // (:540-547).  A call is 1 + 3 launches of the SDF kernel and one of the SDF-gradient kernel.  Round 3 still writes its samples' points, default SDF
    // (100 in every slot: what k_ray_merge_any carries along when NI != NFIX), occupancy bytes and list: a depths-only form of the round was measured
    // and not kept (profiles/NOTES.md, round 10).
    RoundArgs ra{};
    ra.g = RayGeom{io->rays_o, io->rays_d, R};
    ra.z = z; ra.sdf = sdf; ra.msk = msk; ra.maskvol = io->maskvol; ra.D = io->D;
    ra.new_z = new_z; ra.new_sdf = new_sdf; ra.new_msk = new_msk;
    ra.n_imp = (int)NI; ra.out_z = new_z; ra.out_pts = pts; ra.out_sdf = new_sdf; ra.out_msk = new_msk; ra.list = list;
    int cur = NS;
    for (int i = 0; i < 4; ++i) {
        ra.S = cur; ra.n_new = i ? (int)NI : 0; ra.inv_s = 64.f * (float)(1 << i); ra.count = counters + RC_ROUND + i; ra.done = counters + RC_DONE + i;
        ra.seg_rays = G; ra.n_seg = n_seg; ra.seg_cnt = G ? segc + (size_t)i * n_seg : nullptr; ra.seg_prev = (G && i) ? segc + (size_t)(i - 1) * n_seg : nullptr;
        if ((rc = ray_round_launch(RM_UPSAMPLE, ra, wbuf, stream))) return rc;             // incl. cat_z_vals' "more than one point" rule (round_epilogue)
        cur += ra.n_new;
        if (i < 3 && (rc = sdf_eval(0, pts, list, counters + RC_ROUND + i, 0, new_sdf, nullptr))) return rc;      // round 3: nobody reads that SDF
    }
    int* count = counters + RC_FINAL;            // occupied mid-points: what the network kernels evaluate
    // :484 -- the caller passes the mean over the rays for per-ray near / far; the scalar form is (far - near) / n_samples
    const float sample_dist = io->sample_dist > 0.f ? io->sample_dist : (io->far - io->near) / (float)NS;
    float* fpts = pts;   // reuse
    // the last cat_z_vals fused with render_core's head
    ra.S = cur; ra.n_new = (int)NI; ra.count = count; ra.done = counters + RC_DONE + 4; ra.sample_dist = sample_dist;
    ra.seg_cnt = G ? segc + (size_t)4 * n_seg : nullptr; ra.seg_prev = G ? segc + (size_t)3 * n_seg : nullptr;
    ra.mid_z = io->mid_z; ra.dists = io->dists; ra.pts = fpts; ra.pm = io->pm; ra.o_sdf = io->sdf; ra.grad = io->grad; ra.rgb = io->rgb; ra.defaults_everywhere = 0;
    if ((rc = ray_round_launch(RM_FINALIZE, ra, nullptr, stream))) return rc;               // incl. render_core's "first 100 points" rule (round_epilogue)
    const bool cull = io->weight_cull > 0.f;
    const bool sorts = render_sorts_list(R, NS, NIMP, io->V);
    int* slist = lay.at<int>(workspace, lay.sorted_list);
    // the list grouped by view-visibility signature (stable): the colour kernel then skips every (tile, view) pair in which no point sees the view instead of
    // 3/4 of them -- 40.0 -> 36.1 ms at 8 views, bit-identical results (csrc/list_sort.hip); only for lists long enough to pay for it (render_sorts_list).
    // The SDF-gradient kernel does not care about the order (10.17 vs 10.15 ms): with weight culling it runs on the emission-order list and only the
    // (shorter) culled list is sorted.
    auto sort_list = [&](const int* in, const int* n_dev) {
        return o2345_list_sort_by_visibility(fpts, in, n_dev, (long long)(S * RR), io->proj, io->V, io->H, io->W, slist, nullptr, lay.at<void>(workspace, lay.sort_ws),
                                             lay.sort_ws.bytes, stream);
    };
    const int* clist = list;                     // what the colour network evaluates
    const int* ccount = count;
    const float* counted_elsewhere = io->pm;     // slots whose valid-view count the colour kernel writes itself
    if (!cull && sorts) {
        if ((rc = sort_list(list, count))) return rc;
        list = slist; clist = slist;
    }
    if ((rc = sdf_eval(2, fpts, list, count, 0, io->sdf, io->grad))) return rc;
    if (cull) {
        int* list2 = lay.at<int>(workspace, lay.cull_list);
        int* count2 = counters + RC_CULLED;
        float* keep = sdf;                       // the workspace's SDF list is dead after the last merge
        const size_t lds = group_lds_bytes(CULL_ARRAYS, (int)S);
        if (use_group_form(R, lds))
            hipLaunchKernelGGL(k_ray_cull_group, dim3(cdiv(R, GR)), dim3(64), lds, s, ra.g, (int)S, io->dists, io->pm, io->sdf, io->grad, io->inv_s, io->alpha_inter_ratio,
                               io->weight_cull, keep, io->rgb, list2, count2);
        else
            hipLaunchKernelGGL(k_ray_cull, dim3(cdiv(R, 256)), dim3(256), 0, s, ra.g, (int)S, io->dists, io->pm, io->sdf, io->grad, io->inv_s, io->alpha_inter_ratio,
                               io->weight_cull, keep, io->rgb, list2, count2);
        if ((rc = check_launch("ray_cull"))) return rc;
        clist = list2; ccount = count2; counted_elsewhere = keep;
        if (sorts) {
            if ((rc = sort_list(list2, count2))) return rc;
            clist = slist;
        }
    }
    // valid-view counts (feed the per-ray colour mask): the colour kernels write them for the points they evaluate (the occupied ones, 88 % at
    // BASELINE config 2); this pass covers the rest (four IEEE divisions per view make it VALU-bound: 0.48 ms over all points)
    if ((rc = o2345_view_count_unlisted(fpts, (long long)S * R, counted_elsewhere, io->maskvol, io->D, io->proj, io->V, io->H, io->W, io->nviews, stream))) return rc;
    // the colour kernel's tile queue: eight of the call's counters (O2345_TILE_QUEUE=0: none, the static schedule)
    rc = color_points_launch(io->color_x3_blob != nullptr, io->color_x3_blob ? io->color_x3_blob : io->color_mfma_blob, io->vol_cl, io->maskvol, io->D, io->cmaps, io->proj,
                             io->cam_pos, io->V, io->H, io->W, fpts, clist, ccount, 0, io->query_cam, nullptr, io->rgb, io->nviews, io->color_stats,
                             knobs().tile_queue ? counters + RC_QUEUE : nullptr, stream);
    if (rc) return rc;
    if ((rc = o2345_ray_composite(io->rays_o, io->rays_d, R, (int)S, io->mid_z, io->dists, io->pm, io->sdf, io->grad, io->rgb, io->nviews, io->inv_s, io->alpha_inter_ratio, io->background,
                                  io->color, io->depth, io->weights, io->cdf, io->weights_sum, io->weights_max, io->depth_var, io->alpha_sum, io->grad_err, io->color_mask, stream))) return rc;
    if (io->scalars) hipLaunchKernelGGL(k_ray_scalars, dim3(G ? n_seg : 1), dim3(1024), 0, s, R, (int)S, io->alpha_sum, io->grad_err, G ? segc + (size_t)4 * n_seg : count,
                                        io->scalars, G);
    if (io->z_vals) O2345_HIP(hipMemcpyAsync(io->z_vals, z, S * RR * sizeof(float), hipMemcpyDeviceToDevice, s));
    return check_launch("render_rays");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_render() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)(k_quirk_min2));
}
}  // namespace o2345
