// The grid object of a target mesh (built by mesh_distance.hip, walked by its query, by mesh_align.hip, by mesh_intersect.hip and by mesh_raycast.hip): its one layout, the limit
// on its cells, and the two closest-triangle searches of one point (through the grid, and over every triangle) that the distance query and the alignment
// step share -- one text, so the step's d2 and nearest are the query's bits by construction.
#pragma once
#include "mesh_common.h"
#include "mesh_distance_math.h"

namespace o2345 {

constexpr long long MD_MAX_CELLS = 1ll << 24;
constexpr int MD_AXIS = 256;                          // cells per axis at most
constexpr long long MD_MAX_SAMPLES = 1ll << 28;
constexpr int MD_RED_ITEMS = 16;                      // samples per thread of the fixed-order sums (k_md_reduce, k_ma_step)
constexpr int MD_RED_TILE = 256 * MD_RED_ITEMS;
constexpr double MD_SLACK = 9.313225746154785e-10;    // 2^-30
constexpr double MD_DOWN = 0.9999999999990905;        // 1 - 2^-40: a product rounded towards zero, and then some

// the grid object: head (128 bytes), then cell_start [max_cells + 1], then the entries
struct MdGridObject {
    MdGridHead* head;
    int *cell_start, *entries;
};

inline size_t md_grid_object(void* grid, long long max_cells, long long n_entries, MdGridObject& g) {
    Carver w(grid);
    g.head = w.take_bytes<MdGridHead>(128);
    g.cell_start = w.take<int>(max_cells + 1);
    g.entries = w.take<int>(n_entries);
    return w.bytes();
}

// what a walker that does not trust the grid reads of it (the pair test of mesh_intersect.hip, the segment walk of mesh_raycast.hip): entries and cells
// are clamped to the sizes the caller states, so a grid of another mesh gives wrong results, not a fault
struct MdGridView {
    const MdGridHead* head;
    const int *cell_start, *entries;
    long long cap_entries, max_cells;
};

// the grid argument of an entry -> the view; grid NULL: the exhaustive path, for at most exhaustive_max triangles.  false: refused (the error is set)
inline bool md_grid_view(const char* unit, const void* grid, size_t grid_bytes, long long max_cells, long long nt, long long exhaustive_max, MdGridView& g) {
    g = MdGridView{};
    if (!grid) {
        if (nt > exhaustive_max) { set_error("%s: %lld triangles without a grid; the exhaustive path takes at most %lld", unit, nt, exhaustive_max); return false; }
        return true;
    }
    if (max_cells < 1 || max_cells > MD_MAX_CELLS) { set_error("%s: a grid needs its max_cells (1 .. 2^24), got %lld", unit, max_cells); return false; }
    MdGridObject o;
    const size_t need = md_grid_object(const_cast<void*>(grid), max_cells, 0, o);
    if (grid_bytes < need || ((uintptr_t)grid & 15) != 0) { set_error("%s: grid of %zu bytes (at least %zu, 16-byte aligned)", unit, grid_bytes, need); return false; }
    const long long cap = (long long)((grid_bytes - need) / sizeof(int));
    g.head = o.head; g.cell_start = o.cell_start; g.entries = o.entries;
    g.cap_entries = cap < (1ll << 31) - 1 ? cap : (1ll << 31) - 1;
    g.max_cells = max_cells;
    return true;
}

// the corners of a triangle whose indices are in range -> true iff all nine coordinates are finite
__device__ __forceinline__ bool md_corners(const double* __restrict__ verts, int a, int b, int c, double (&A)[3], double (&B)[3], double (&C)[3]) {
    bool all_finite = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        A[d] = verts[3 * (long long)a + d]; B[d] = verts[3 * (long long)b + d]; C[d] = verts[3 * (long long)c + d];
        all_finite &= finite(A[d]) && finite(B[d]) && finite(C[d]);
    }
    return all_finite;
}

template <typename IDX>
__device__ __forceinline__ void md_visit_cell(int ci, const int* __restrict__ cell_start, const int* __restrict__ entries, const double* __restrict__ verts, int nv,
                                              const IDX* __restrict__ tris, const double (&p)[3], double& best, int& best_t) {
    const int e1 = cell_start[ci + 1];
    for (int e = cell_start[ci]; e < e1; ++e) {
        const int t = entries[e];
        int a, b, c, region;
        (void)mesh_triangle(tris, t, nv, a, b, c);                   // registered: usable
        double A[3], B[3], C[3];
        (void)md_corners(verts, a, b, c, A, B, C);
        const double d2 = md_point_triangle(p, A, B, C, region);
        if (d2 < best || (d2 == best && t < best_t)) { best = d2; best_t = t; }
    }
}

// the closest triangle of p through the grid: shells of cells around the point's own cell (see "walk" in mesh_distance.hip) -> best = d2, best_t = nearest
template <typename IDX>
__device__ __forceinline__ void md_walk_grid(const double (&p)[3], const double* __restrict__ verts, int nv, const IDX* __restrict__ tris,
                                             const MdGridHead* __restrict__ head, const int* __restrict__ cell_start, const int* __restrict__ entries,
                                             double& best_out, int& best_t_out) {
    const double cell = head->cell;
    const int nx = head->dims[0], ny = head->dims[1], nz = head->dims[2];
    const double ox = head->origin[0], oy = head->origin[1], oz = head->origin[2];
    const int cx = md_cell_index(p[0], ox, cell, nx), cy = md_cell_index(p[1], oy, cell, ny), cz = md_cell_index(p[2], oz, cell, nz);
    const double slack = (head->scale + fmax(fabs(p[0]), fmax(fabs(p[1]), fabs(p[2])))) * MD_SLACK;
    double best = INFINITY;                                          // locals, written out once: updated through the references the query takes 103 VGPRs, not 93
    int best_t = -1;
    const int rmax = max(max(max(cx, nx - 1 - cx), max(cy, ny - 1 - cy)), max(cz, nz - 1 - cz));
    for (int r = 0; r <= rmax; ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1), x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1);
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const int rowi = (z * ny + y) * nx;
                if (abs(z - cz) == r || abs(y - cy) == r) {
                    for (int x = x0; x <= x1; ++x) md_visit_cell(rowi + x, cell_start, entries, verts, nv, tris, p, best, best_t);
                } else {                                             // inside the shell's z and y range: its two x faces
                    if (cx - r >= 0) md_visit_cell(rowi + cx - r, cell_start, entries, verts, nv, tris, p, best, best_t);
                    if (cx + r < nx) md_visit_cell(rowi + cx + r, cell_start, entries, verts, nv, tris, p, best, best_t);
                }
            }
        // the closest that anything outside the cube of shells 0 .. r can be
        double lb = INFINITY;
        if (cx + r + 1 < nx) lb = fmin(lb, (ox + (double)(cx + r + 1) * cell) - p[0]);
        if (cx - r > 0) lb = fmin(lb, p[0] - (ox + (double)(cx - r) * cell));
        if (cy + r + 1 < ny) lb = fmin(lb, (oy + (double)(cy + r + 1) * cell) - p[1]);
        if (cy - r > 0) lb = fmin(lb, p[1] - (oy + (double)(cy - r) * cell));
        if (cz + r + 1 < nz) lb = fmin(lb, (oz + (double)(cz + r + 1) * cell) - p[2]);
        if (cz - r > 0) lb = fmin(lb, p[2] - (oz + (double)(cz - r) * cell));
        lb = lb - slack;
        if (lb > 0.0 && (lb * lb) * MD_DOWN > best) break;
    }
    best_out = best;
    best_t_out = best_t;
}

// the closest triangle of p among all nt, in index order: the definition on the device, and the path for tiny targets
template <typename IDX>
__device__ __forceinline__ void md_walk_all(const double (&p)[3], const double* __restrict__ verts, int nv, const IDX* __restrict__ tris, long long nt,
                                            double& best_out, int& best_t_out) {
    double best = INFINITY;
    int best_t = -1;
    for (long long t = 0; t < nt; ++t) {
        int a, b, c, region;
        if (!mesh_triangle(tris, t, nv, a, b, c)) continue;
        double A[3], B[3], C[3];
        if (!md_corners(verts, a, b, c, A, B, C)) continue;
        if (md_normal2(A, B, C) == 0.0) continue;
        const double d2 = md_point_triangle(p, A, B, C, region);
        if (d2 < best) { best = d2; best_t = (int)t; }
    }
    best_out = best;
    best_t_out = best_t;
}

// fixed-order sums of N values over a 256-thread block: wave butterflies, then (w0 + w1) + (w2 + w3); valid in thread 0.  The butterfly is written
// out: these are doubles, and its order is part of the result (wave_sum is for integers)
template <int N>
__device__ __forceinline__ void md_block_sums(double (&v)[N]) {
    __shared__ double sm[N][4];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        for (int off = 32; off; off >>= 1) v[k] += __shfl_xor(v[k], off);
        if ((threadIdx.x & 63) == 0) sm[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = (sm[k][0] + sm[k][1]) + (sm[k][2] + sm[k][3]);
    }
}

}  // namespace o2345
