// One step of aligning mesh A to mesh B by a similarity transform, on the device: for each of K candidate transforms, A's samples are moved, matched to
// their closest triangle of B, and the moments of the point-to-plane Gauss-Newton system are summed -- one fused pass (k_ma_step) and one fold
// (k_ma_final).  The 7 x 7 solve and the loop stay on the host (mesh_io.similarity_step / align_meshes, shared with the host twin, which is the definition).
//
// Definitions
//   pair       (transform k, sample e): x = ma_apply(T_k, p_e); its closest triangle of B by the distance query's own walk (md_walk_grid / md_walk_all,
//              mesh_grid.h): d2 and nearest are o2345_mesh_distance_query's bits of x by construction; q = md_closest_point on that triangle.
//   matched    nearest >= 0 and d2 finite and >= 0; inlier: matched and (tau == 0 or d2 <= tau tau), tau = max_distance.  Without a target (tris NULL) every
//              sample is an inlier with q = x and d2 = 0, and columns 0 .. 34 stay 0: columns 35 and 39 .. 42 then give the centroid and the rms radius
//              of a sample set.
//   row        48 doubles per transform: 0 .. 27 the upper triangle of sum w J J^T, row-major; 28 .. 34 sum w J b (ma_jacobian / ma_terms, over the inliers);
//              35 sum w and 36 sum w d2 over the inliers; 37 sum w and 38 sum w min(d2, tau tau) over the matched; 39 .. 41 sum w x' and 42 sum w |x'|^2
//              over the inliers, x' = x - pivot; 43, 44, 45 the numbers of inliers, rejected and unmatched samples; 46, 47 zero.
//   sums       the distance unit's scheme per transform: a thread adds its MD_RED_ITEMS consecutive samples in index order, a block folds its 256 threads in
//              the written-out tree (md_block_sums) into one row of partials, and one block per transform folds the rows (256 sequential chains, the same
//              tree).  The longest chain of additions is 16 + 8 + n / 2^20 + 8 <= 288; no floating-point atomics: the same bytes on every run.
// Bad input never faults: a target index outside [0, nv) or a non-finite target coordinate is skipped as the query skips it, never dereferenced.
#include "mesh_grid.h"
#include "mesh_align_math.h"

namespace o2345 {

enum { MA_NO_TARGET = 0, MA_ALL = 1, MA_GRID = 2 };

struct MaPivot { double c[3], tau; };

// block (b, k): samples [b * MD_RED_TILE, (b + 1) * MD_RED_TILE) under transform k, thread i its MD_RED_ITEMS consecutive ones -> partials[k][b][MA_COLS]
template <typename IDX, int MODE>
__global__ __launch_bounds__(256) void k_ma_step(const double* __restrict__ points, const double* __restrict__ weights, long long n,
                                                 const double* __restrict__ transforms, const double* __restrict__ verts, int nv, const IDX* __restrict__ tris,
                                                 long long nt, const MdGridHead* __restrict__ head, const int* __restrict__ cell_start,
                                                 const int* __restrict__ entries, MaPivot pv, double* __restrict__ partials, double* __restrict__ moved,
                                                 double* __restrict__ d2_out, int* __restrict__ nearest_out) {
    const int k = blockIdx.y;
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = transforms[12 * k + i];
    const double tau2 = pv.tau * pv.tau;
    double v[MA_SUMS];
#pragma unroll
    for (int i = 0; i < MA_SUMS; ++i) v[i] = 0.0;
    const long long first = ((long long)blockIdx.x * 256 + threadIdx.x) * MD_RED_ITEMS;
#pragma unroll 1
    for (int j = 0; j < MD_RED_ITEMS; ++j) {
        const long long e = first + j;
        if (e >= n) break;
        const double p[3] = {points[3 * e], points[3 * e + 1], points[3 * e + 2]};
        double x[3], best = 0.0;
        int best_t = -1;
        ma_apply(T, p, x);
        if constexpr (MODE == MA_GRID) md_walk_grid(x, verts, nv, tris, head, cell_start, entries, best, best_t);
        if constexpr (MODE == MA_ALL) md_walk_all(x, verts, nv, tris, nt, best, best_t);
        const long long at = (long long)k * n + e;
        if (moved) { moved[3 * at] = x[0]; moved[3 * at + 1] = x[1]; moved[3 * at + 2] = x[2]; }
        if (d2_out) d2_out[at] = best;
        if (nearest_out) nearest_out[at] = best_t;
        if (MODE != MA_NO_TARGET && !(best_t >= 0 && best >= 0.0 && best <= DBL_MAX)) { v[45] = v[45] + 1.0; continue; }
        const double w = weights ? weights[e] : 1.0;
        const bool inlier = pv.tau == 0.0 || best <= tau2;
        v[37] = v[37] + w;
        v[38] = v[38] + w * (inlier ? best : tau2);
        if (!inlier) { v[44] = v[44] + 1.0; continue; }
        double xp[3];
        md_sub(x, pv.c, xp);
        v[35] = v[35] + w;
        v[36] = v[36] + w * best;
#pragma unroll
        for (int d = 0; d < 3; ++d) v[39 + d] = v[39 + d] + w * xp[d];
        v[42] = v[42] + w * md_dot(xp, xp);
        v[43] = v[43] + 1.0;
        if constexpr (MODE != MA_NO_TARGET) {
            int a, b, c, region;
            (void)mesh_triangle(tris, best_t, nv, a, b, c);          // the walk's answer: usable
            double A[3], B[3], C[3], q[3], J[7], rhs, term[MA_TERMS];
            (void)md_corners(verts, a, b, c, A, B, C);
            (void)md_closest_point(x, A, B, C, region, q);
            ma_jacobian(x, q, A, B, C, pv.c, J, rhs);
            ma_terms(J, rhs, w, term);
#pragma unroll
            for (int i = 0; i < MA_TERMS; ++i) v[i] = v[i] + term[i];
        }
    }
    md_block_sums(v);
    if (threadIdx.x == 0) {
        double* row = partials + ((long long)k * gridDim.x + blockIdx.x) * MA_COLS;
#pragma unroll
        for (int i = 0; i < MA_COLS; ++i) row[i] = i < MA_SUMS ? v[i] : 0.0;
    }
}

// block k: thread i adds rows i, i + 256, ... of transform k in that order, then the block's tree -> moments[k][MA_COLS]
__global__ __launch_bounds__(256) void k_ma_final(const double* __restrict__ partials, long long rows, double* __restrict__ moments) {
    const int k = blockIdx.x;
    double v[MA_SUMS];
#pragma unroll
    for (int i = 0; i < MA_SUMS; ++i) v[i] = 0.0;
    for (long long r = threadIdx.x; r < rows; r += 256) {
        const double* row = partials + ((long long)k * rows + r) * MA_COLS;
#pragma unroll
        for (int i = 0; i < MA_SUMS; ++i) v[i] = v[i] + row[i];
    }
    md_block_sums(v);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < MA_COLS; ++i) moments[(long long)k * MA_COLS + i] = i < MA_SUMS ? v[i] : 0.0;
    }
}

struct MaCarve {
    double* partials;
    long long rows;
};

static bool ma_sizes_ok(long long n, int n_transforms) { return n >= 0 && n < MD_MAX_SAMPLES && n_transforms >= 1 && n_transforms <= MA_MAX_TRANSFORMS; }

static size_t ma_carve(void* ws, long long n, int n_transforms, MaCarve& c) {
    c.rows = (n + MD_RED_TILE - 1) / MD_RED_TILE;
    Carver w(ws);
    c.partials = w.take<double>((size_t)(c.rows ? c.rows : 1) * n_transforms * MA_COLS);          // never empty: 0 bytes means bad sizes
    return w.bytes();
}

}  // namespace o2345

using namespace o2345;

extern "C" {

size_t o2345_mesh_align_workspace_bytes(long long n, int n_transforms) {
    if (!ma_sizes_ok(n, n_transforms)) return 0;
    MaCarve c;
    return ma_carve(nullptr, n, n_transforms, c);
}

int o2345_mesh_align_step(const double* points, const double* weights, long long n, const double* transforms, int n_transforms, const double* verts,
                          const void* tris, int index_bytes, long long nv, long long nt, const void* grid, size_t grid_bytes, long long max_cells,
                          double max_distance, double pivot_x, double pivot_y, double pivot_z, void* workspace, size_t workspace_bytes, double* moments,
                          double* moved, double* d2, int* nearest, void* stream) {
    O2345_REQUIRE(n >= 0 && n < MD_MAX_SAMPLES, "mesh_align_step: bad sample count %lld (n < 2^28)", n);
    O2345_REQUIRE(n_transforms >= 1 && n_transforms <= MA_MAX_TRANSFORMS, "mesh_align_step: n_transforms must be in 1 .. 64, got %d", n_transforms);
    O2345_REQUIRE(max_distance >= 0.0 && max_distance <= DBL_MAX, "mesh_align_step: max_distance must be finite and >= 0 (0: no truncation), got %g", max_distance);
    O2345_REQUIRE(o2345::finite(pivot_x) && o2345::finite(pivot_y) && o2345::finite(pivot_z), "mesh_align_step: the pivot must be finite");
    O2345_REQUIRE(transforms && moments && (n == 0 || points), "mesh_align_step: null pointer");
    O2345_REQUIRE_WORKSPACE("mesh_align_step", workspace, workspace_bytes, o2345_mesh_align_workspace_bytes(n, n_transforms));
    if (tris) {
        O2345_REQUIRE_INDEX_BYTES("mesh_align_step", index_bytes);
        O2345_REQUIRE(mesh_sizes_ok(nv, nt) && (nv == 0 || verts), "mesh_align_step: bad target (nv < 2^30, 3 * nt < 2^31)");
    } else {
        O2345_REQUIRE(!grid, "mesh_align_step: a grid needs a target");
        index_bytes = 4;
    }
    MdGridObject g = {};
    if (grid) {
        O2345_REQUIRE(nt > 0 && max_cells >= 1 && max_cells <= MD_MAX_CELLS, "mesh_align_step: a grid needs a target and its max_cells");
        const size_t need = md_grid_object(nullptr, max_cells, 0, g);
        O2345_REQUIRE(grid_bytes >= need && ((uintptr_t)grid & 15) == 0, "mesh_align_step: grid of %zu bytes (at least %zu, 16-byte aligned)", grid_bytes, need);
        (void)md_grid_object(const_cast<void*>(grid), max_cells, 0, g);
    }
    hipStream_t s = (hipStream_t)stream;
    // the transforms are few: checked on the host, which costs one synchronisation of the stream (the caller reads the moments back after every step anyway)
    double T[MA_MAX_TRANSFORMS * 12];
    hipError_t e = hipMemcpyAsync(T, transforms, (size_t)n_transforms * 12 * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    O2345_REQUIRE(e == hipSuccess, "mesh_align_step: %s", hipGetErrorString(e));
    for (int i = 0; i < 12 * n_transforms; ++i)
        O2345_REQUIRE(o2345::finite(T[i]), "mesh_align_step: transform %d has a non-finite entry", i / 12);
    MaCarve c;
    (void)ma_carve(workspace, n, n_transforms, c);
    const MaPivot pv = {{pivot_x, pivot_y, pivot_z}, max_distance};
    if (c.rows) {
        const dim3 blocks((unsigned)c.rows, (unsigned)n_transforms);
        with_index_type(index_bytes, tris, [&](auto* t) {
            using IDX = index_type<decltype(t)>;
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, blocks, dim3(256), 0, s, points, weights, n, transforms, verts, (int)nv, t, nt, g.head, g.cell_start, g.entries, pv,
                                   c.partials, moved, d2, nearest);
            };
            if (!tris) launch(k_ma_step<IDX, MA_NO_TARGET>);
            else if (grid) launch(k_ma_step<IDX, MA_GRID>);
            else launch(k_ma_step<IDX, MA_ALL>);
        });
    }
    hipLaunchKernelGGL(k_ma_final, dim3((unsigned)n_transforms), dim3(256), 0, s, c.partials, c.rows, moments);
    return check_launch("mesh_align_step");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_mesh_align() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)k_ma_final);
}
}  // namespace o2345
