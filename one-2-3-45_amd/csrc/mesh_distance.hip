// Distance between two triangle meshes as surfaces, on the device: area-weighted surface samples of one mesh (k_md_levels, k_md_emit), a uniform grid
// over the other (k_md_grid_*), the closest triangle of every sample through that grid (k_md_query_grid) or exhaustively (k_md_query_all), and the
// summary of one direction (k_md_reduce, k_md_reduce_final).  Samples, d2 and nearest equal the host twin (mesh_io.surface_samples / closest_triangles)
// to the last bit: fp64, one operation at a time, in a defined order (mesh_distance_math.h), or integer.
//
// Definitions
//   samples    triangle t at `spacing` has level k_t (md_level; 1 without a spacing) and k_t^2 samples at the centroids of its regular split (md_sample),
//              each of weight area_t / k_t^2; samples are numbered triangle-major through the exclusive scan of k_t^2.  Fewer than 2^28 in all.
//   target     a triangle takes part as a target iff its three indices lie in [0, nv), its nine coordinates are finite and n . n != 0 ("usable").
//   d2         the minimum of md_point_triangle over the usable triangles; nearest: the smallest index among those that attain it; +inf and -1 when no
//              triangle is usable.
//   grid       cells are boxes of the lattice of multiples of `cell`; a usable triangle is registered in every cell its bounding box touches, through
//              the one monotone index function md_cell_index, which also places the query.  cell = 0 asks for the default: about as many cells as
//              usable triangles.  An edge that would give more than 256 cells along an axis or more than max_cells in all is enlarged (x 1.25 at a
//              time) until it does not.  Per-cell lists are ascending by triangle index.
//   walk       the query visits the shells of cells at Chebyshev distance r = 0, 1, ... around its own (clamped) cell.  A triangle not seen after shell
//              r is registered only in cells outside that cube, so along some axis and side every point q of it has a cell index beyond the cube's
//              face.  Because the index function is monotone and rounds by at most a few 2^-53 of the coordinates, q lies beyond the plane
//              origin + m cell up to such an error, and the COMPUTED closest point of md_point_triangle is a convex combination of the corners up to
//              the same kind of error.  The walk stops when the smallest of the up to six plane distances, minus a slack of 2^-30 of the largest
//              coordinate involved (a million times those errors; one more shell costs little), is positive and its square, rounded towards zero,
//              exceeds the best d2 found.  The result is therefore the exhaustive kernel's, bit for bit, whatever the cell edge.
//   summary    over the samples with a finite d2 >= 0 and a nearest >= 0 (the others are counted in n_unmatched): W = sum w, sum w d, sum w d^2 and
//              sum w [d <= tau] with d = sqrt(d2), the largest d2 as its bit pattern, and the counts.  Sums: every thread adds MD_RED_ITEMS terms in
//              index order, a block folds its 256 threads in a fixed tree into one row of partials, and one block folds the rows (256 sequential chains,
//              the same tree).  The longest chain of additions is 16 + 8 + n / 2^20 + 8 <= 288: a relative error of at most 3.2e-14 for the
//              non-negative terms, and the same bits on every run.  No floating-point atomics anywhere.
// Bad input never faults: an index outside [0, nv) is counted and never dereferenced, a non-finite coordinate is counted; count() returns them as errors.
#include "mesh_grid.h"

namespace o2345 {

constexpr int MD_THRESHOLDS = sizeof(O2345DistanceStats::within) / sizeof(double);          // 8 (the device block of the reduction: include/o2345.h)
constexpr int MD_RED_COLS = 3 + MD_THRESHOLDS;        // sum w, sum w d, sum w d^2, within[8]

struct MdThresholds { double tau[MD_THRESHOLDS]; int n; };

// device scalars of a samples call (workspace head)
struct MdSampleTotals {
    long long scan_total;
    unsigned long long n_samples, n_bad, n_nonfinite;
};

// device scalars of a grid call (workspace head)
struct MdGridTotals {
    unsigned long long lo[3], hi[3];                  // ordered_bits of the bounds of the usable triangles' corners
    unsigned long long n_bad, n_nonfinite, n_degenerate, n_usable;
    long long n_entries;                              // written by k_scan_small
    int n_long;
};
static_assert(sizeof(MdSampleTotals) <= 128 && sizeof(MdGridTotals) <= 128 && sizeof(MdGridHead) <= 128, "the heads are 128 bytes");

// ---- samples -------------------------------------------------------------------------------------------------------------------------------------
// kk[t] = k_t^2 (1 for a triangle that is counted as bad input); the 64-bit total is an integer atomic: the int scan may wrap where it exceeds 2^28
template <typename IDX>
__global__ __launch_bounds__(256) void k_md_levels(const double* __restrict__ verts, int nv, const IDX* __restrict__ tris, long long nt, double spacing,
                                                   int* __restrict__ kk, MdSampleTotals* __restrict__ tot) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false, nonfinite = false;
    unsigned long long mine = 0;
    if (t < nt) {
        int a, b, c, k = 1;
        if (!mesh_triangle(tris, t, nv, a, b, c)) bad = true;
        else {
            double A[3], B[3], C[3];
            if (!md_corners(verts, a, b, c, A, B, C)) nonfinite = true;
            else k = md_level(A, B, C, spacing);
        }
        kk[t] = k * k;
        mine = (unsigned long long)(k * k);
    }
    wave_count(bad, &tot->n_bad);
    wave_count(nonfinite, &tot->n_nonfinite);
    mine = wave_sum(mine);
    if (lane_id() == 0 && mine) atomicAdd(&tot->n_samples, mine);
}

// thread per sample: its triangle by bisection of the offsets
template <typename IDX>
__global__ __launch_bounds__(256) void k_md_emit(const double* __restrict__ verts, int nv, const IDX* __restrict__ tris, long long nt, const int* __restrict__ kk,
                                                 const int* __restrict__ off, long long n, double* __restrict__ points, double* __restrict__ weights,
                                                 int* __restrict__ triangle) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    long long lo = 0, hi = nt - 1;                                   // the last t with off[t] <= e
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if ((long long)off[mid] <= e) lo = mid; else hi = mid - 1;
    }
    const long long t = lo;
    const int k2 = kk[t];
    int k = (int)(sqrtf((float)k2) + 0.5f);
    int s = (int)(e - (long long)off[t]);
    if (s >= k2) s = k2 - 1;                                         // only after an error status of count()
    double p[3] = {0.0, 0.0, 0.0}, w = 0.0;
    int a, b, c;
    if (mesh_triangle(tris, t, nv, a, b, c)) {
        double A[3], B[3], C[3];
        (void)md_corners(verts, a, b, c, A, B, C);
        md_sample(A, B, C, k, s, p);
        w = md_weight(A, B, C, k);
    }
    if (points) { points[3 * e] = p[0]; points[3 * e + 1] = p[1]; points[3 * e + 2] = p[2]; }
    if (weights) weights[e] = w;
    if (triangle) triangle[e] = (int)t;
}

// ---- grid ----------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_md_grid_init(int* __restrict__ cellcnt, long long n_cellcnt, MdGridTotals* __restrict__ tot) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        MdGridTotals z = {};
        for (int d = 0; d < 3; ++d) z.lo[d] = ~0ull;
        *tot = z;
    }
    if (i < n_cellcnt) cellcnt[i] = 0;
}

// usable[t], the bounds of the usable triangles' corners, and the counters
template <typename IDX>
__global__ __launch_bounds__(256) void k_md_grid_bounds(const double* __restrict__ verts, int nv, const IDX* __restrict__ tris, long long nt,
                                                        unsigned char* __restrict__ usable, MdGridTotals* __restrict__ tot) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false, nonfinite = false, degenerate = false, ok = false;
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
    if (t < nt) {
        int a, b, c;
        if (!mesh_triangle(tris, t, nv, a, b, c)) bad = true;
        else {
            double A[3], B[3], C[3];
            if (!md_corners(verts, a, b, c, A, B, C)) nonfinite = true;
            else if (md_normal2(A, B, C) == 0.0) degenerate = true;
            else {
                ok = true;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    lo[d] = ordered_bits(fmin(A[d], fmin(B[d], C[d])));
                    hi[d] = ordered_bits(fmax(A[d], fmax(B[d], C[d])));
                }
            }
        }
        if (usable) usable[t] = ok ? 1 : 0;
    }
    wave_count(bad, &tot->n_bad);
    wave_count(nonfinite, &tot->n_nonfinite);
    wave_count(degenerate, &tot->n_degenerate);
    wave_count(ok, &tot->n_usable);
    if (!usable) return;                                             // the reduce entry wants the counters only
    const unsigned long long any = __ballot(ok);
#pragma unroll
    for (int d = 0; d < 3; ++d) { lo[d] = wave_min(lo[d]); hi[d] = wave_max(hi[d]); }
    if (lane_id() == 0 && any) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { atomicMin(&tot->lo[d], lo[d]); atomicMax(&tot->hi[d], hi[d]); }
    }
}

// one thread: the cell edge, the origin and the cells per axis from the bounds
__global__ void k_md_grid_head(const MdGridTotals* __restrict__ tot, double cell, long long max_cells, MdGridHead* __restrict__ head) {
    if (blockIdx.x || threadIdx.x) return;
    MdGridHead h = {};
    h.cell = 1.0;
    h.dims[0] = h.dims[1] = h.dims[2] = 1;
    if (tot->n_usable) {
        double lo[3], hi[3], widest = 0.0;
        for (int d = 0; d < 3; ++d) { lo[d] = ordered_double(tot->lo[d]); hi[d] = ordered_double(tot->hi[d]); widest = fmax(widest, hi[d] - lo[d]); }
        double c = cell > 0.0 ? cell : (widest > 0.0 ? widest / (double)MD_AXIS : 1.0);
        const double want = cell > 0.0 ? (double)max_cells : fmin((double)max_cells, (double)tot->n_usable);
        for (int it = 0; it < 400; ++it) {
            double nd[3], o[3];
            bool fits = true;
            for (int d = 0; d < 3; ++d) {
                o[d] = floor(lo[d] / c) * c;
                nd[d] = floor((hi[d] - o[d]) / c) + 1.0;
                fits &= nd[d] >= 1.0 && nd[d] <= (double)MD_AXIS;
            }
            if (fits && nd[0] * nd[1] * nd[2] <= want) {
                h.cell = c;
                for (int d = 0; d < 3; ++d) { h.origin[d] = o[d]; h.dims[d] = (int)nd[d]; }
                break;
            }
            c = c * 1.25;                                            // never fitting (an overflowing extent) leaves the single cell: slow, not wrong
        }
    }
    h.n_cells = h.dims[0] * h.dims[1] * h.dims[2];
    for (int d = 0; d < 3; ++d) h.scale = fmax(h.scale, fmax(fabs(h.origin[d]), fabs(h.origin[d] + (double)h.dims[d] * h.cell)));
    *head = h;
}

// FILL false: cellcnt[c] += 1 for every cell the bounding box of usable triangle t touches; true: entries[cursor[c]++] = t
template <typename IDX, bool FILL>
__global__ __launch_bounds__(256) void k_md_grid_register(const double* __restrict__ verts, int nv, const IDX* __restrict__ tris, long long nt,
                                                          const unsigned char* __restrict__ usable, const MdGridHead* __restrict__ head,
                                                          int* __restrict__ counter, int* __restrict__ entries, long long n_entries) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt || !usable[t]) return;
    int a, b, c;
    (void)mesh_triangle(tris, t, nv, a, b, c);                       // usable: in range
    double A[3], B[3], C[3];
    (void)md_corners(verts, a, b, c, A, B, C);
    int c0[3], c1[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        c0[d] = md_cell_index(fmin(A[d], fmin(B[d], C[d])), head->origin[d], head->cell, head->dims[d]);
        c1[d] = md_cell_index(fmax(A[d], fmax(B[d], C[d])), head->origin[d], head->cell, head->dims[d]);
    }
    const int nx = head->dims[0], ny = head->dims[1];
    for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) {
                const int ci = (z * ny + y) * nx + x;
                const int at = atomicAdd(counter + ci, 1);
                if (FILL && at < n_entries) entries[at] = (int)t;          // at < n_entries unless the caller passed another count than count() gave
            }
}

// one thread per cell: short rows are sorted here, long ones are listed
__global__ __launch_bounds__(256) void k_md_grid_rows(const MdGridHead* __restrict__ head, const int* __restrict__ cell_start, int* __restrict__ entries,
                                                      int* __restrict__ long_list, MdGridTotals* __restrict__ tot) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= head->n_cells) return;
    const int lo = cell_start[c], d = cell_start[c + 1] - lo;
    if (d > ROW_SHORT) long_list[atomicAdd(&tot->n_long, 1)] = (int)c;
    else if (d > 1) row_sort_short(entries + lo, d);
}

// one block per listed row: odd-even transposition in place, d passes (a cell with thousands of triangles: a grid far too coarse for its mesh).  Not
// row_sort_long: that needs a second buffer of the entries' size, and the grid's workspace and object have none (their sizes are part of the interface)
__global__ __launch_bounds__(256) void k_md_grid_long_rows(const int* __restrict__ cell_start, int* entries, const int* __restrict__ long_list,
                                                           const MdGridTotals* __restrict__ tot) {
    const int n_long = tot->n_long;
    for (int r = blockIdx.x; r < n_long; r += gridDim.x) {
        const int c = long_list[r];
        const int lo = cell_start[c], d = cell_start[c + 1] - lo;
        int* row = entries + lo;
        for (int pass = 0; pass < d; ++pass) {
            for (int i = 2 * (int)threadIdx.x + (pass & 1); i + 1 < d; i += 512) {
                const int x = row[i], y = row[i + 1];
                if (x > y) { row[i] = y; row[i + 1] = x; }
            }
            __syncthreads();
        }
    }
}

// the grid object: head, then cell_start [max_cells + 1] (entries follow, written by the register and row kernels)
__global__ __launch_bounds__(256) void k_md_grid_finish(const MdGridHead* __restrict__ head, const MdGridTotals* __restrict__ tot, const int* __restrict__ cell_start,
                                                        long long n_start, long long cell_start_bytes, MdGridHead* __restrict__ out_head, int* __restrict__ out_start) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        MdGridHead h = *head;
        h.n_entries = tot->n_entries;
        h.cell_start_bytes = cell_start_bytes;
        *out_head = h;
    }
    if (i < n_start) out_start[i] = cell_start[i];
}

// ---- query ---------------------------------------------------------------------------------------------------------------------------------------
// one lane per point: shells of cells around the point's own cell (md_walk_grid, mesh_grid.h; see "walk" above)
template <typename IDX>
__global__ __launch_bounds__(256) void k_md_query_grid(const double* __restrict__ pts, long long n, const double* __restrict__ verts, int nv,
                                                       const IDX* __restrict__ tris, const MdGridHead* __restrict__ head, const int* __restrict__ cell_start,
                                                       const int* __restrict__ entries, double* __restrict__ d2_out, int* __restrict__ nearest_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    double best;
    int best_t;
    md_walk_grid(p, verts, nv, tris, head, cell_start, entries, best, best_t);
    d2_out[i] = best;
    nearest_out[i] = best_t;
}

// one lane per point against every triangle in index order (md_walk_all, mesh_grid.h): the definition on the device, and the path for tiny targets
template <typename IDX>
__global__ __launch_bounds__(256) void k_md_query_all(const double* __restrict__ pts, long long n, const double* __restrict__ verts, int nv,
                                                      const IDX* __restrict__ tris, long long nt, double* __restrict__ d2_out, int* __restrict__ nearest_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    double best;
    int best_t;
    md_walk_all(p, verts, nv, tris, nt, best, best_t);
    d2_out[i] = best;
    nearest_out[i] = best_t;
}

// ---- summary -------------------------------------------------------------------------------------------------------------------------------------
// (the fixed-order block sums, md_block_sums, are in mesh_grid.h: the alignment step adds its moments by the same tree)
// block b: samples [b * MD_RED_TILE, (b + 1) * MD_RED_TILE), thread i its MD_RED_ITEMS consecutive ones -> partials[b][MD_RED_COLS]
__global__ __launch_bounds__(256) void k_md_reduce(const double* __restrict__ d2, const int* __restrict__ nearest, const double* __restrict__ weights, long long n,
                                                   MdThresholds th, double* __restrict__ partials, O2345DistanceStats* __restrict__ st) {
    double v[MD_RED_COLS];
#pragma unroll
    for (int k = 0; k < MD_RED_COLS; ++k) v[k] = 0.0;
    unsigned long long mx = 0;
    int unmatched = 0;
    const long long first = ((long long)blockIdx.x * 256 + threadIdx.x) * MD_RED_ITEMS;
    for (int j = 0; j < MD_RED_ITEMS; ++j) {
        const long long e = first + j;
        if (e >= n) break;
        const double x = d2[e];
        if (!(x >= 0.0 && x <= DBL_MAX) || (nearest && nearest[e] < 0)) { ++unmatched; continue; }
        const double w = weights ? weights[e] : 1.0;
        const double d = sqrt(x);
        v[0] = v[0] + w;
        v[1] = v[1] + w * d;
        v[2] = v[2] + w * x;
#pragma unroll
        for (int k = 0; k < MD_THRESHOLDS; ++k)
            if (k < th.n && d <= th.tau[k]) v[3 + k] = v[3 + k] + w;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
        mx = bits > mx ? bits : mx;
    }
    mx = wave_max(mx);
    const unsigned long long um = wave_sum((unsigned long long)unmatched);
    if (lane_id() == 0) {
        if (mx) atomicMax(&st->max_d2_bits, mx);
        if (um) atomicAdd(&st->n_unmatched, um);
    }
    md_block_sums(v);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < MD_RED_COLS; ++k) partials[(long long)blockIdx.x * MD_RED_COLS + k] = v[k];
    }
}

// one block: thread i adds rows i, i + 256, ... in that order, then the block's tree
__global__ __launch_bounds__(256) void k_md_reduce_final(const double* __restrict__ partials, long long rows, long long n, O2345DistanceStats* __restrict__ st) {
    double v[MD_RED_COLS];
#pragma unroll
    for (int k = 0; k < MD_RED_COLS; ++k) v[k] = 0.0;
    for (long long r = threadIdx.x; r < rows; r += 256) {
#pragma unroll
        for (int k = 0; k < MD_RED_COLS; ++k) v[k] = v[k] + partials[r * MD_RED_COLS + k];
    }
    md_block_sums(v);
    if (threadIdx.x == 0) {
        st->sum_w = v[0]; st->sum_wd = v[1]; st->sum_wd2 = v[2];
#pragma unroll
        for (int k = 0; k < MD_THRESHOLDS; ++k) st->within[k] = v[3 + k];
        st->n = (unsigned long long)n;
    }
}

// the target's bad-input counters of the summary
__global__ __launch_bounds__(64) void k_md_reduce_target(const MdGridTotals* __restrict__ tot, O2345DistanceStats* __restrict__ st) {
    if (blockIdx.x || threadIdx.x) return;
    st->n_degenerate = tot->n_degenerate;
    st->n_bad = tot->n_bad + tot->n_nonfinite;
}

// ---- workspaces ----------------------------------------------------------------------------------------------------------------------------------
struct MdSampleCarve {
    MdSampleTotals* tot;
    int *kk, *off, *block;
    unsigned nb;
};

static size_t md_sample_carve(void* ws, long long nt, MdSampleCarve& c) {
    c.nb = cdiv(nt, SCAN_TILE);
    Carver w(ws);
    c.tot = w.take_bytes<MdSampleTotals>(128);
    c.kk = w.take<int>(nt);
    c.off = w.take<int>(nt);
    c.block = w.take<int>(c.nb);
    return w.bytes();
}

struct MdGridCarve {
    MdGridTotals* tot;
    MdGridHead* head;
    int *cellcnt, *cell_start, *cursor, *long_list, *block;
    unsigned char* usable;
    long long n_start;                                               // max_cells + 1: the scanned array ends with the total
    unsigned nb;
};

static bool md_grid_ok(long long nt, long long max_cells) { return nt >= 0 && 3 * nt < (1ll << 31) && max_cells >= 1 && max_cells <= MD_MAX_CELLS; }

static size_t md_grid_carve(void* ws, long long nt, long long max_cells, MdGridCarve& c) {
    c.n_start = max_cells + 1;
    c.nb = cdiv(c.n_start, SCAN_TILE);
    Carver w(ws);
    c.tot = w.take_bytes<MdGridTotals>(128);
    c.head = w.take_bytes<MdGridHead>(128);
    for (int** a : {&c.cellcnt, &c.cell_start, &c.cursor}) *a = w.take<int>(c.n_start);
    c.long_list = w.take<int>(max_cells);
    c.block = w.take<int>(c.nb);
    c.usable = w.take<unsigned char>(nt);
    return w.bytes();
}

struct MdReduceCarve {
    MdGridTotals* tot;
    double* partials;
    long long rows;
};

static size_t md_reduce_carve(void* ws, long long n, MdReduceCarve& c) {
    c.rows = (n + MD_RED_TILE - 1) / MD_RED_TILE;
    Carver w(ws);
    c.tot = w.take_bytes<MdGridTotals>(128);
    c.partials = w.take<double>(c.rows * MD_RED_COLS);
    return w.bytes();
}

}  // namespace o2345

using namespace o2345;

extern "C" {

size_t o2345_mesh_samples_workspace_bytes(long long nt) {
    if (nt < 0 || 3 * nt >= (1ll << 31)) return 0;
    MdSampleCarve c;
    return md_sample_carve(nullptr, nt, c);
}

int o2345_mesh_samples_count(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, double spacing, void* workspace,
                             size_t workspace_bytes, long long* n_samples_host, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_samples_count", index_bytes);
    O2345_REQUIRE(spacing >= 0.0 && spacing <= DBL_MAX, "mesh_samples_count: spacing must be a finite float > 0, or 0 for one sample per triangle, got %g", spacing);
    O2345_REQUIRE(mesh_sizes_ok(nv, nt), "mesh_samples_count: bad sizes (nv must stay below 2^30 and 3 * nt below 2^31)");
    O2345_REQUIRE(n_samples_host && (nv == 0 || verts) && (nt == 0 || tris), "mesh_samples_count: null pointer");
    O2345_REQUIRE_WORKSPACE("mesh_samples_count", workspace, workspace_bytes, o2345_mesh_samples_workspace_bytes(nt));
    MdSampleCarve c;
    (void)md_sample_carve(workspace, nt, c);
    hipStream_t s = (hipStream_t)stream;
    O2345_HIP(hipMemsetAsync(c.tot, 0, 128, s));
    if (nt > 0) {
        with_index_type(index_bytes, tris, [&](auto* t) {
            hipLaunchKernelGGL(k_md_levels<index_type<decltype(t)>>, dim3(cdiv(nt, 256)), dim3(256), 0, s, verts, (int)nv, t, nt, spacing, c.kk, c.tot);
        });
        exclusive_scan<SCAN_ITEMS>(c.kk, nt, c.nb, c.block, c.off, nullptr, &c.tot->scan_total, s);
    }
    int rc = check_launch("mesh_samples_count");
    if (rc) return rc;
    MdSampleTotals h;
    if ((rc = read_totals(h, c.tot, s, "mesh_samples_count"))) return rc;
    O2345_REQUIRE(h.n_bad == 0, "mesh_samples_count: %llu triangles index outside 0 .. %lld", h.n_bad, nv - 1);
    O2345_REQUIRE(h.n_nonfinite == 0, "mesh_samples_count: %llu triangles have a non-finite vertex coordinate", h.n_nonfinite);
    O2345_REQUIRE(h.n_samples < (unsigned long long)MD_MAX_SAMPLES, "mesh_samples_count: %llu samples; the limit is 2^28 - 1 (raise the spacing)", h.n_samples);
    *n_samples_host = (long long)h.n_samples;
    return 0;
}

int o2345_mesh_samples_emit(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, void* workspace, long long n_samples,
                            double* points, double* weights, int* triangle, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_samples_emit", index_bytes);
    O2345_REQUIRE(mesh_sizes_ok(nv, nt), "mesh_samples_emit: bad sizes");
    O2345_REQUIRE(n_samples >= 0 && n_samples < MD_MAX_SAMPLES && (nt > 0 || n_samples == 0), "mesh_samples_emit: bad sample count %lld", n_samples);
    O2345_REQUIRE(workspace && (n_samples == 0 || (verts && tris)), "mesh_samples_emit: null pointer");
    if (n_samples == 0) return 0;
    MdSampleCarve c;
    (void)md_sample_carve(workspace, nt, c);
    hipStream_t s = (hipStream_t)stream;
    with_index_type(index_bytes, tris, [&](auto* t) {
        hipLaunchKernelGGL(k_md_emit<index_type<decltype(t)>>, dim3(cdiv(n_samples, 256)), dim3(256), 0, s, verts, (int)nv, t, nt, c.kk, c.off, n_samples, points,
                           weights, triangle);
    });
    return check_launch("mesh_samples_emit");
}

size_t o2345_mesh_distance_grid_workspace_bytes(long long nt, long long max_cells) {
    if (!md_grid_ok(nt, max_cells)) return 0;
    MdGridCarve c;
    return md_grid_carve(nullptr, nt, max_cells, c);
}

size_t o2345_mesh_distance_grid_bytes(long long max_cells, long long n_entries) {
    if (max_cells < 1 || max_cells > MD_MAX_CELLS || n_entries < 0 || n_entries >= (1ll << 31)) return 0;
    MdGridObject g;
    return md_grid_object(nullptr, max_cells, n_entries, g);
}

int o2345_mesh_distance_grid_count(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, double cell, long long max_cells,
                                   void* workspace, size_t workspace_bytes, long long* n_entries_host, long long* n_degenerate_host, int* dims_host,
                                   double* cell_host, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_distance_grid_count", index_bytes);
    O2345_REQUIRE(cell >= 0.0 && cell <= DBL_MAX, "mesh_distance_grid_count: cell must be a finite float > 0, or 0 for the default, got %g", cell);
    O2345_REQUIRE(mesh_sizes_ok(nv, nt) && md_grid_ok(nt, max_cells), "mesh_distance_grid_count: bad sizes (nv < 2^30, 3 * nt < 2^31, max_cells in [1, 2^24])");
    O2345_REQUIRE(n_entries_host && (nv == 0 || verts) && (nt == 0 || tris), "mesh_distance_grid_count: null pointer");
    O2345_REQUIRE_WORKSPACE("mesh_distance_grid_count", workspace, workspace_bytes, o2345_mesh_distance_grid_workspace_bytes(nt, max_cells));
    MdGridCarve c;
    (void)md_grid_carve(workspace, nt, max_cells, c);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_md_grid_init, dim3(cdiv(c.n_start, 256)), dim3(256), 0, s, c.cellcnt, c.n_start, c.tot);
    with_index_type(index_bytes, tris, [&](auto* t) {
        using IDX = index_type<decltype(t)>;
        if (nt > 0) hipLaunchKernelGGL(k_md_grid_bounds<IDX>, dim3(cdiv(nt, 256)), dim3(256), 0, s, verts, (int)nv, t, nt, c.usable, c.tot);
        hipLaunchKernelGGL(k_md_grid_head, dim3(1), dim3(64), 0, s, c.tot, cell, max_cells, c.head);
        if (nt > 0) hipLaunchKernelGGL((k_md_grid_register<IDX, false>), dim3(cdiv(nt, 256)), dim3(256), 0, s, verts, (int)nv, t, nt, c.usable, c.head, c.cellcnt, nullptr, 0ll);
    });
    exclusive_scan<SCAN_ITEMS>(c.cellcnt, c.n_start, c.nb, c.block, c.cell_start, c.cursor, &c.tot->n_entries, s);
    int rc = check_launch("mesh_distance_grid_count");
    if (rc) return rc;
    MdGridTotals h;
    MdGridHead hh;
    if ((rc = read_totals(h, c.tot, s, "mesh_distance_grid_count"))) return rc;
    if ((rc = read_totals(hh, c.head, s, "mesh_distance_grid_count"))) return rc;
    O2345_REQUIRE(h.n_bad == 0, "mesh_distance_grid_count: %llu triangles index outside 0 .. %lld", h.n_bad, nv - 1);
    O2345_REQUIRE(h.n_nonfinite == 0, "mesh_distance_grid_count: %llu triangles have a non-finite vertex coordinate", h.n_nonfinite);
    O2345_REQUIRE(h.n_usable > 0, "mesh_distance_grid_count: the target has no triangle with an area (%lld triangles, %llu degenerate)", nt, h.n_degenerate);
    O2345_REQUIRE(h.n_entries >= 0 && h.n_entries < (1ll << 31), "mesh_distance_grid_count: %lld cell entries; the limit is 2^31 - 1 (raise the cell edge)", h.n_entries);
    *n_entries_host = h.n_entries;
    if (n_degenerate_host) *n_degenerate_host = (long long)h.n_degenerate;
    if (dims_host) for (int d = 0; d < 3; ++d) dims_host[d] = hh.dims[d];
    if (cell_host) *cell_host = hh.cell;
    return 0;
}

int o2345_mesh_distance_grid_emit(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, long long max_cells, void* workspace,
                                  long long n_entries, void* grid, size_t grid_bytes, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_distance_grid_emit", index_bytes);
    O2345_REQUIRE(mesh_sizes_ok(nv, nt) && md_grid_ok(nt, max_cells) && nt > 0, "mesh_distance_grid_emit: bad sizes");
    O2345_REQUIRE(workspace && grid && verts && tris, "mesh_distance_grid_emit: null pointer");
    const size_t need = o2345_mesh_distance_grid_bytes(max_cells, n_entries);
    O2345_REQUIRE(need && grid_bytes >= need, "mesh_distance_grid_emit: grid of %zu bytes, need %zu", grid_bytes, need);
    O2345_REQUIRE(((uintptr_t)grid & 15) == 0, "mesh_distance_grid_emit: grid must be 16-byte aligned");
    MdGridCarve c;
    (void)md_grid_carve(workspace, nt, max_cells, c);
    MdGridObject g;
    (void)md_grid_object(grid, max_cells, n_entries, g);
    hipStream_t s = (hipStream_t)stream;
    O2345_HIP(hipMemcpyAsync(c.cursor, c.cell_start, (size_t)c.n_start * sizeof(int), hipMemcpyDeviceToDevice, s));      // a second emit starts over
    O2345_HIP(hipMemsetAsync(&c.tot->n_long, 0, sizeof(int), s));
    with_index_type(index_bytes, tris, [&](auto* t) {
        using IDX = index_type<decltype(t)>;
        hipLaunchKernelGGL((k_md_grid_register<IDX, true>), dim3(cdiv(nt, 256)), dim3(256), 0, s, verts, (int)nv, t, nt, c.usable, c.head, c.cursor, g.entries, n_entries);
    });
    hipLaunchKernelGGL(k_md_grid_rows, dim3(cdiv(max_cells, 256)), dim3(256), 0, s, c.head, c.cell_start, g.entries, c.long_list, c.tot);
    hipLaunchKernelGGL(k_md_grid_long_rows, dim3(ROW_LONG_GRID), dim3(256), 0, s, c.cell_start, g.entries, c.long_list, c.tot);
    hipLaunchKernelGGL(k_md_grid_finish, dim3(cdiv(c.n_start, 256)), dim3(256), 0, s, c.head, c.tot, c.cell_start, c.n_start,
                       (long long)((char*)g.entries - (char*)g.cell_start), g.head, g.cell_start);
    return check_launch("mesh_distance_grid_emit");
}

int o2345_mesh_distance_query(const double* points, long long n, const double* verts, const void* tris, int index_bytes, long long nv, long long nt,
                              const void* grid, size_t grid_bytes, long long max_cells, double* d2, int* nearest, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_distance_query", index_bytes);
    O2345_REQUIRE(mesh_sizes_ok(nv, nt) && n >= 0 && n < MD_MAX_SAMPLES, "mesh_distance_query: bad sizes (nv < 2^30, 3 * nt < 2^31, n < 2^28)");
    O2345_REQUIRE((n == 0 || (points && d2 && nearest)) && (nv == 0 || verts) && (nt == 0 || tris), "mesh_distance_query: null pointer");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (grid) {
        O2345_REQUIRE(nt > 0 && max_cells >= 1 && max_cells <= MD_MAX_CELLS, "mesh_distance_query: a grid needs a target and its max_cells");
        const size_t need = o2345_mesh_distance_grid_bytes(max_cells, 0);
        O2345_REQUIRE(grid_bytes >= need && ((uintptr_t)grid & 15) == 0, "mesh_distance_query: grid of %zu bytes (at least %zu, 16-byte aligned)", grid_bytes, need);
        MdGridObject g;
        (void)md_grid_object(const_cast<void*>(grid), max_cells, 0, g);
        with_index_type(index_bytes, tris, [&](auto* t) {
            hipLaunchKernelGGL(k_md_query_grid<index_type<decltype(t)>>, dim3(cdiv(n, 256)), dim3(256), 0, s, points, n, verts, (int)nv, t, g.head, g.cell_start, g.entries,
                               d2, nearest);
        });
    } else {
        with_index_type(index_bytes, tris, [&](auto* t) {
            hipLaunchKernelGGL(k_md_query_all<index_type<decltype(t)>>, dim3(cdiv(n, 256)), dim3(256), 0, s, points, n, verts, (int)nv, t, nt, d2, nearest);
        });
    }
    return check_launch("mesh_distance_query");
}

size_t o2345_mesh_distance_reduce_workspace_bytes(long long n) {
    if (n < 0 || n >= MD_MAX_SAMPLES) return 0;
    MdReduceCarve c;
    return md_reduce_carve(nullptr, n, c);
}

int o2345_mesh_distance_reduce(const double* d2, const int* nearest, const double* weights, long long n, const double* thresholds, int n_thresholds,
                               const double* verts, const void* tris, int index_bytes, long long nv, long long nt, void* workspace, size_t workspace_bytes,
                               O2345DistanceStats* stats, void* stream) {
    O2345_REQUIRE(n >= 0 && n < MD_MAX_SAMPLES, "mesh_distance_reduce: bad sample count %lld", n);
    O2345_REQUIRE(n_thresholds >= 0 && n_thresholds <= MD_THRESHOLDS && (n_thresholds == 0 || thresholds), "mesh_distance_reduce: %d thresholds; at most 8", n_thresholds);
    O2345_REQUIRE(stats && workspace && (n == 0 || d2), "mesh_distance_reduce: null pointer");
    O2345_REQUIRE(!tris || ((index_bytes == 4 || index_bytes == 8) && mesh_sizes_ok(nv, nt) && (nv == 0 || verts)), "mesh_distance_reduce: bad target");
    O2345_REQUIRE(workspace_bytes >= o2345_mesh_distance_reduce_workspace_bytes(n), "mesh_distance_reduce: workspace too small");
    O2345_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)stats & 7) == 0, "mesh_distance_reduce: workspace must be 16-byte and stats 8-byte aligned");
    MdThresholds th = {};
    th.n = n_thresholds;
    for (int k = 0; k < n_thresholds; ++k) {
        O2345_REQUIRE(thresholds[k] >= 0.0 && thresholds[k] <= DBL_MAX, "mesh_distance_reduce: threshold %d must be finite and >= 0, got %g", k, thresholds[k]);
        th.tau[k] = thresholds[k];
    }
    MdReduceCarve c;
    (void)md_reduce_carve(workspace, n, c);
    hipStream_t s = (hipStream_t)stream;
    O2345_HIP(hipMemsetAsync(stats, 0, sizeof *stats, s));
    O2345_HIP(hipMemsetAsync(c.tot, 0, 128, s));
    if (c.rows) hipLaunchKernelGGL(k_md_reduce, dim3((unsigned)c.rows), dim3(256), 0, s, d2, nearest, weights, n, th, c.partials, stats);
    hipLaunchKernelGGL(k_md_reduce_final, dim3(1), dim3(256), 0, s, c.partials, c.rows, n, stats);
    if (tris && nt > 0) {
        with_index_type(index_bytes, tris, [&](auto* t) {
            hipLaunchKernelGGL(k_md_grid_bounds<index_type<decltype(t)>>, dim3(cdiv(nt, 256)), dim3(256), 0, s, verts, (int)nv, t, nt, (unsigned char*)nullptr, c.tot);
        });
        hipLaunchKernelGGL(k_md_reduce_target, dim3(1), dim3(64), 0, s, c.tot, stats);
    }
    return check_launch("mesh_distance_reduce");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_mesh_distance() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)k_md_reduce_final);
}
}  // namespace o2345
