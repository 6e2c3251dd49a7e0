// Projection of mesh vertices onto a level set of the neural SDF on the device: a few Newton steps p <- p - (s - level) g / |g|^2 per vertex, with the
// SDF and its analytic gradient from the library's own network kernels.  Equal to the host twin (mesh_io.project_vertices) to the last bit when the twin
// is handed the same kernels as its field: everything outside the network is fp64, one operation at a time, in a defined order, and has no square root.
//
// Definitions (R = grid_R, bmin / bmax the float32 bounds widened to fp64, ext = bmax - bmin; index units: one grid spacing = 1)
//   world      w_k = x_k / (R - 1) * ext_k + bmin_k; the network sees float32(w) -- for (-1, 1) the pipeline's verts_idx / (R - 1) * 2 - 1 to the bit.
//   a round    evaluates (s, g) at the float32 world point of every ACTIVE vertex (all of them in round 0), then per vertex, o its input position and
//              x its current one:  r = |double(s) - level|;
//              s or g non-finite, or g2 = (gx gx + gy gy) + gz gz not > 0  -> STALLED, leaves the active set, keeps x;
//              else r <= tol                                                -> CONVERGED, leaves, keeps x;
//              else, in rounds 0 .. iterations - 1:  t = (double(s) - level) / g2;  d_k = t g_k;  e_k = d_k / ext_k * (R - 1), clamped to
//              [-max_step, max_step] per axis;  y_k = x_k - e_k, clamped to [o_k - max_move, o_k + max_move], then to [0, R - 1];  x <- y.  Each of the
//              three clamps that changes a value counts one `clamped` event (up to nine per vertex and round);
//              else (round `iterations`, which only classifies)             -> UNCONVERGED.
//   maxima     max_before = max of r in round 0; max_after = max of the r at which the vertices left or ended; non-finite r do not take part.
//   Not promised: that a vertex stays on its sheet of the surface beyond the max_move box, or that triangles keep their orientation where the surface
//   folds inside one cell.
//
// Why list order does not matter.  The active list of the next round is filled through ballots and one integer atomicAdd per block, so its order
// changes between runs; a vertex's slot in every array is its own index, the network kernels scatter through the list (point i is pts[list[i]], results
// go to slot list[i]), and a point's SDF and gradient do not depend on its place in a tile.  The counters are integer atomics, the maxima 64-bit integer
// atomicMax of the bit pattern of a non-negative double (which orders like the double).  No float atomics.  Counter r of the 66 is written before round
// r and read in it, never reused, so the list of counts is also the `evaluated` of the twin.
#include "mesh_math.h"
#include <float.h>

namespace o2345 {

constexpr int PROJ_COUNTS = sizeof(O2345ProjectStats::count) / sizeof(int);       // rounds 0 .. 64 and one behind (the device block of one call: include/o2345.h)
constexpr int PROJ_ITEMS = 4;                         // list entries per thread of k_proj_step
constexpr int PROJ_TILE = 256 * PROJ_ITEMS;           // per block

// thread per vertex: x = the input, its float32 world point, the identity list, the count of round 0; the stats block was zeroed before (memset)
__global__ __launch_bounds__(256) void k_proj_init(const double* __restrict__ verts, int nv, IndexFrame f, double* __restrict__ x, float* __restrict__ pts,
                                                   int* __restrict__ list, O2345ProjectStats* __restrict__ st) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    bool nonfinite = false;
    if (v == 0) st->count[0] = nv;
    if (v < nv) {
        double p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = verts[3 * v + k];
            nonfinite |= !finite(p[k]);
            x[3 * v + k] = p[k];
        }
        index_to_world_f32(p, f, pts + 3 * v);
        list[v] = (int)v;
    }
    wave_count(nonfinite, &st->n_nonfinite);
}

// Every thread takes PROJ_ITEMS entries of this round's list, a block PROJ_TILE consecutive ones: classify, step, and append the survivors to the other
// list.  Counters and maxima are reduced over the block first (wave shuffles, then LDS), so that a block issues at most one atomic per counter and one
// atomicAdd for its place in the next list: with one set of atomics per wave the 3,250 waves of a 200,000-vertex round spent 95 us queueing on the
// stats block's two cache lines.
__global__ __launch_bounds__(256) void k_proj_step(const double* __restrict__ origin, int nv, double* __restrict__ x, float* __restrict__ pts,
                                                   const float* __restrict__ sdf, const float* __restrict__ grad, const int* __restrict__ list,
                                                   int* __restrict__ next, O2345ProjectStats* __restrict__ st, int round, int last, IndexFrame f, double level,
                                                   double tol, double max_step, double max_move) {
    __shared__ int wave_tot[5], red_n[4][4], list_base;
    __shared__ unsigned long long red_m[4][2];
    int n = st->count[round];
    n = n < nv ? n : nv;
    const long long first = (long long)blockIdx.x * PROJ_TILE;
    if (first >= n) return;                                         // the whole block
    int vs[PROJ_ITEMS];
    bool survives[PROJ_ITEMS];
    int n_converged = 0, n_stalled = 0, n_unconverged = 0, clamps = 0;
    unsigned long long before = 0ull, after = 0ull;                 // bit patterns of finite r; 0 takes no part in a maximum
#pragma unroll
    for (int k = 0; k < PROJ_ITEMS; ++k) {
        const long long i = first + k * 256 + threadIdx.x;
        vs[k] = 0;
        survives[k] = false;
        if (i >= n) continue;
        const long long v = list[i];
        vs[k] = (int)v;
        const float s32 = sdf[v], g32[3] = {grad[3 * v], grad[3 * v + 1], grad[3 * v + 2]};
        const bool net_finite = fabsf(s32) <= FLT_MAX && fabsf(g32[0]) <= FLT_MAX && fabsf(g32[1]) <= FLT_MAX && fabsf(g32[2]) <= FLT_MAX;
        const double g[3] = {(double)g32[0], (double)g32[1], (double)g32[2]};
        const double ds = __dsub_rn((double)s32, level);
        const double r = fabs(ds);
        const double g2 = __dadd_rn(__dadd_rn(__dmul_rn(g[0], g[0]), __dmul_rn(g[1], g[1])), __dmul_rn(g[2], g[2]));
        const unsigned long long rbits = finite(r) ? (unsigned long long)__double_as_longlong(r) : 0ull;
        if (round == 0) before = rbits > before ? rbits : before;
        if (!net_finite || !(g2 > 0.0)) ++n_stalled;
        else if (r <= tol) ++n_converged;
        else if (last) ++n_unconverged;
        else {
            survives[k] = true;
            const double t = __ddiv_rn(ds, g2);
            double y[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                double e = __dmul_rn(__ddiv_rn(__dmul_rn(t, g[d]), f.bext[d]), f.rm1);
                if (e < -max_step) { e = -max_step; ++clamps; } else if (e > max_step) { e = max_step; ++clamps; }
                const double o = origin[3 * v + d];
                const double lo = __dsub_rn(o, max_move), hi = __dadd_rn(o, max_move);
                double q = __dsub_rn(x[3 * v + d], e);
                if (q < lo) { q = lo; ++clamps; } else if (q > hi) { q = hi; ++clamps; }
                if (q < 0.0) { q = 0.0; ++clamps; } else if (q > f.rm1) { q = f.rm1; ++clamps; }
                y[d] = q;
                x[3 * v + d] = q;
            }
            index_to_world_f32(y, f, pts + 3 * v);
        }
        if (!survives[k]) after = rbits > after ? rbits : after;
    }
    // the survivors' places inside the block, item after item (the order of a list is arbitrary, its content is not)
    int pos[PROJ_ITEMS], total = 0;
#pragma unroll
    for (int k = 0; k < PROJ_ITEMS; ++k) {
        int tk;
        pos[k] = total + block_prefix<4>(survives[k], wave_tot, tk);
        total += tk;
    }
    n_converged = wave_sum(n_converged); n_stalled = wave_sum(n_stalled); n_unconverged = wave_sum(n_unconverged); clamps = wave_sum(clamps);
    before = wave_max(before); after = wave_max(after);
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) {
        red_n[w][0] = n_converged; red_n[w][1] = n_stalled; red_n[w][2] = n_unconverged; red_n[w][3] = clamps;
        red_m[w][0] = before; red_m[w][1] = after;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c[4] = {0, 0, 0, 0};
        unsigned long long m[2] = {0ull, 0ull};
        for (int j = 0; j < 4; ++j) {
            for (int q = 0; q < 4; ++q) c[q] += red_n[j][q];
            for (int q = 0; q < 2; ++q) m[q] = red_m[j][q] > m[q] ? red_m[j][q] : m[q];
        }
        if (c[0]) atomicAdd(&st->converged, (unsigned long long)c[0]);
        if (c[1]) atomicAdd(&st->stalled, (unsigned long long)c[1]);
        if (c[2]) atomicAdd(&st->unconverged, (unsigned long long)c[2]);
        if (c[3]) atomicAdd(&st->clamped, (unsigned long long)c[3]);
        if (m[0]) atomicMax(&st->max_before, m[0]);
        if (m[1]) atomicMax(&st->max_after, m[1]);
        list_base = total ? atomicAdd(&st->count[round + 1], total) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PROJ_ITEMS; ++k) {
        const long long slot = (long long)list_base + pos[k];
        if (survives[k] && slot < nv) next[slot] = vs[k];          // always in range: the survivors are a subset of this round's list
    }
}

struct ProjCarve {
    float *pts, *sdf, *grad;
    int* list[2];
};

static bool proj_size_ok(long long nv) { return nv >= 0 && nv < (1ll << 30); }

// the one walk through the workspace: carves it, or sizes it when ws is null; returns its size
static size_t proj_carve(void* ws, long long nv, ProjCarve& c) {
    Carver w(ws);
    c.pts = w.take<float>(nv * 3);
    c.grad = w.take<float>(nv * 3);
    c.sdf = w.take<float>(nv);
    c.list[0] = w.take<int>(nv);
    c.list[1] = w.take<int>(nv);
    return w.bytes();
}

static bool proj_positive(double x) { return x > 0.0 && finite(x); }

}  // namespace o2345

using namespace o2345;

extern "C" {

size_t o2345_mesh_project_workspace_bytes(long long nv) {
    if (!proj_size_ok(nv)) return 0;
    ProjCarve c;
    const size_t b = proj_carve(nullptr, nv, c);
    return b ? b : 16;
}

// All rounds are queued at once: the count of every round's list stays on the device (the network kernels take it as n_dev).  No host synchronisation.
int o2345_mesh_project(const float* blob, const float* vol_cl, int D, int sdf_mode, const double* verts, long long nv, int grid_R, const float* bound_min,
                       const float* bound_max, int iterations, double level, double tol, double max_step, double max_move, void* workspace,
                       size_t workspace_bytes, double* verts_out, O2345ProjectStats* stats, void* stream) {
    O2345_REQUIRE(sdf_mode == 0 || sdf_mode == 2, "mesh_project: sdf_mode must be 0 (fp32) or 2 (split-f16), got %d", sdf_mode);
    O2345_REQUIRE(proj_size_ok(nv), "mesh_project: bad size (nv must be in [0, 2^30))");
    O2345_REQUIRE(grid_R >= 2, "mesh_project: bad resolution %d", grid_R);
    O2345_REQUIRE(iterations >= 1 && iterations <= PROJ_COUNTS - 2, "mesh_project: iterations must be in [1, 64], got %d", iterations);
    O2345_REQUIRE(o2345::finite(level), "mesh_project: level must be finite, got %g", level);
    O2345_REQUIRE(tol >= 0.0 && o2345::finite(tol), "mesh_project: tol must be finite and >= 0, got %g", tol);
    O2345_REQUIRE(proj_positive(max_step), "mesh_project: max_step must be finite and > 0, got %g", max_step);
    O2345_REQUIRE(proj_positive(max_move), "mesh_project: max_move must be finite and > 0, got %g", max_move);
    O2345_REQUIRE(bound_min && bound_max && stats && workspace, "mesh_project: null pointer");
    O2345_REQUIRE(nv == 0 || (blob && vol_cl && verts && verts_out), "mesh_project: null pointer");
    O2345_REQUIRE(nv == 0 || verts != verts_out, "mesh_project: verts_out must not be verts (the input is the centre of the max_move box)");
    O2345_REQUIRE(nv == 0 || D >= 2, "mesh_project: bad volume side %d", D);
    O2345_REQUIRE(workspace_bytes >= o2345_mesh_project_workspace_bytes(nv), "mesh_project: workspace too small");
    O2345_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)stats & 7) == 0, "mesh_project: workspace must be 16-byte and stats 8-byte aligned");
    IndexFrame f;
    if (!index_frame("mesh_project", grid_R, bound_min, bound_max, f)) return -1;
    ProjCarve c;
    (void)proj_carve(workspace, nv, c);
    hipStream_t s = (hipStream_t)stream;
    O2345ProjectStats* st = stats;
    O2345_HIP(hipMemsetAsync(st, 0, sizeof *st, s));
    const int n = (int)nv;
    const unsigned gv = nv ? cdiv(nv, 256) : 1;
    hipLaunchKernelGGL(k_proj_init, dim3(gv), dim3(256), 0, s, verts, n, f, verts_out, c.pts, c.list[0], st);
    if (const int rc = check_launch("mesh_project")) return rc;
    if (nv == 0) return 0;
    for (int round = 0; round <= iterations; ++round) {
        const int* list = c.list[round & 1];
        int rc;
        if (sdf_mode == 2) rc = o2345_sdf_grad_x3(blob, vol_cl, D, c.pts, list, st->count + round, nv, 0, 1.f, c.sdf, c.grad, stream);
        else rc = o2345_sdf_mlp_ex(2, blob, vol_cl, D, c.pts, list, st->count + round, nv, 0, 1.f, nullptr, c.sdf, nullptr, nullptr, c.grad, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(k_proj_step, dim3(cdiv(nv, PROJ_TILE)), dim3(256), 0, s, verts, n, verts_out, c.pts, c.sdf, c.grad, list, c.list[(round + 1) & 1], st, round,
                           round == iterations ? 1 : 0, f, level, tol, max_step, max_move);
    }
    return check_launch("mesh_project");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_mesh_project() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)k_proj_step);
}
}  // namespace o2345
