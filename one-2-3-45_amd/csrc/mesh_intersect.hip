// Self-intersections of a triangle mesh on the device: which pairs of triangles cross.  A broad phase over the uniform grid of mesh_distance.hip (or over
// every pair, without a grid) and a narrow phase in fp64 (mesh_intersect_math.h).  Counts, per-face hits and the pair list equal the host twin
// (mesh_io.mesh_intersections) to the last bit, whatever the grid: every decision is a comparison of fp64 values computed one operation at a time in a
// defined order, everything else is integer.
//
// Definitions (include/o2345.h has the full text)
//   part       a face takes part iff its three indices lie in [0, nv), its nine coordinates are finite, n . n != 0 (md_normal2: the grid's "usable") and
//              its three indices are distinct.  The others are skipped and counted.
//   candidate  t < u, both take part, closed bounding boxes overlap on every axis, at most one shared vertex index.
//   intersect  some edge of one face, free of the other's indices, crosses the other strictly (mi_pair_intersects).
// Broad phase.  Two overlapping boxes both contain the point m = max(lo_t, lo_u) (per axis), so both faces are listed in the cell whose index along
// every axis is md_cell_index(m) -- the one monotone function that registered them.  A pair is handled in that cell only: each pair exactly once, no
// dedup pass.  Decomposition: ONE THREAD PER GRID ENTRY (cell, t), which walks the later entries of its ascending row; the work is the sum of k^2 / 2
// over the cells' row lengths k, spread over sum k threads.  (One thread per triangle looping over its cells gives the thread of a triangle that spans
// many cells all of that triangle's work, and revisits a pair in every shared cell before the home-cell rule can drop it in the same way; per entry, the
// longest serial chain is one row.)  The cell of entry e is found by bisection of cell_start.
// Counting and emitting.  k_mi_pairs runs twice.  Pass 1 (count) adds to hits[t], hits[u] and first[t] (the pairs in which t is the smaller face) with
// integer atomics, and to the totals with one atomic per wave; first is scanned into row offsets.  Pass 2 (emit) repeats the search and writes (t, u)
// at row_start[t] + cursor[t]++; the u column of every row is then sorted in place (mesh_common.h's register sorts with a stride of 2, an odd-even
// transposition by one block for a row above ROW_SHORT: the pair array is the only buffer of its size).  t < u, rows ascending by t: the list is
// sorted lexicographically, and its bytes are the same on every run.  No floating-point atomics; no kernel waits for another workgroup or loops until
// nothing changes.
// Bad input never faults: an index outside [0, nv) is counted and never dereferenced, a non-finite coordinate is counted; such faces take no part.  A
// grid that does not belong to the mesh gives wrong counts, not a fault: entries, rows and cells are clamped to the sizes the caller states.
#include "mesh_grid.h"
#include "mesh_intersect_math.h"

namespace o2345 {

constexpr long long MI_EXHAUSTIVE_MAX = 1ll << 16;    // triangles of the path without a grid
constexpr long long MI_MAX_PAIRS = 1ll << 30;

// device scalars of a call (workspace head)
struct MiTotals {
    unsigned long long n_bad, n_nonfinite, n_faces, n_skipped, n_candidates, n_pairs, n_faces_hit, max_hits;
    long long scan_total;                             // written by k_scan_small: the pairs again, through the int scan
    int n_long;
};
static_assert(sizeof(MiTotals) <= 128, "the head is 128 bytes");

struct MiFace {
    int idx[3];
    double P[3][3];
};

// the corners of face t, which takes part
template <typename IDX>
__device__ __forceinline__ void mi_load(const double* __restrict__ verts, int nv, const IDX* __restrict__ tris, long long t, MiFace& f) {
    (void)mesh_triangle(tris, t, nv, f.idx[0], f.idx[1], f.idx[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int d = 0; d < 3; ++d) f.P[k][d] = verts[3 * (long long)f.idx[k] + d];
}

// part[t], box[6 t ..] = lo, hi, and the two per-face counters cleared
template <typename IDX>
__global__ __launch_bounds__(256) void k_mi_faces(const double* __restrict__ verts, int nv, const IDX* __restrict__ tris, long long nt,
                                                  unsigned char* __restrict__ part, double* __restrict__ box, int* __restrict__ hits, int* __restrict__ first,
                                                  MiTotals* __restrict__ tot) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false, nonfinite = false, skipped = false, ok = false;
    if (t < nt) {
        int a, b, c;
        double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
        if (!mesh_triangle(tris, t, nv, a, b, c)) bad = true;
        else {
            double A[3], B[3], C[3];
            bool all_finite = true;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                A[d] = verts[3 * (long long)a + d]; B[d] = verts[3 * (long long)b + d]; C[d] = verts[3 * (long long)c + d];
                all_finite &= finite(A[d]) && finite(B[d]) && finite(C[d]);
            }
            if (!all_finite) nonfinite = true;
            else if (md_normal2(A, B, C) == 0.0 || a == b || b == c || a == c) skipped = true;
            else {
                ok = true;
#pragma unroll
                for (int d = 0; d < 3; ++d) { lo[d] = fmin(A[d], fmin(B[d], C[d])); hi[d] = fmax(A[d], fmax(B[d], C[d])); }
            }
        }
        part[t] = ok ? 1 : 0;
#pragma unroll
        for (int d = 0; d < 3; ++d) { box[6 * t + d] = lo[d]; box[6 * t + 3 + d] = hi[d]; }
        hits[t] = 0;
        first[t] = 0;
    }
    wave_count(bad, &tot->n_bad);
    wave_count(nonfinite, &tot->n_nonfinite);
    wave_count(skipped, &tot->n_skipped);
    wave_count(ok, &tot->n_faces);
}

// t against u > t, both taking part -> 0 nothing, 1 a candidate, 2 an intersecting pair.  HOME: the pair belongs to cell `home` only
template <typename IDX, bool HOME>
__device__ __forceinline__ int mi_test(const double* __restrict__ verts, int nv, const IDX* __restrict__ tris, const double* __restrict__ box, const MiFace& T,
                                       const double (&lo_t)[3], const double (&hi_t)[3], int u, const MdGridHead* __restrict__ head, int home) {
    double lo_u[3], hi_u[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { lo_u[d] = box[6 * (long long)u + d]; hi_u[d] = box[6 * (long long)u + 3 + d]; }
    if (!mi_boxes_overlap(lo_t, hi_t, lo_u, hi_u)) return 0;
    if (HOME) {
        int c[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) c[d] = md_cell_index(fmax(lo_t[d], lo_u[d]), head->origin[d], head->cell, head->dims[d]);
        if ((c[2] * head->dims[1] + c[1]) * head->dims[0] + c[0] != home) return 0;
    }
    MiFace U;
    mi_load(verts, nv, tris, u, U);
    if (mi_shared(T.idx, U.idx) > 1) return 0;
    return mi_pair_intersects(T.idx, T.P, U.idx, U.P) ? 2 : 1;
}

// GRID: one thread per grid entry (cell, t) against the later entries of its row; else one thread per face t against every u > t.  FILL false: the
// counters; true: the pairs at their rows' cursors
template <typename IDX, bool GRID, bool FILL>
__global__ __launch_bounds__(256) void k_mi_pairs(const double* __restrict__ verts, int nv, const IDX* __restrict__ tris, long long nt,
                                                  const unsigned char* __restrict__ part, const double* __restrict__ box, MdGridView g, int* __restrict__ hits,
                                                  int* __restrict__ first, const int* __restrict__ row_start, int* __restrict__ cursor, int* __restrict__ pairs,
                                                  long long n_pairs, MiTotals* __restrict__ tot) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    long long t = -1, j0 = 0, j1 = 0;                  // the face, and the range it is tested against: entries (GRID) or faces
    int home = 0;
    if (GRID) {
        long long n_entries = g.head->n_entries, n_cells = g.head->n_cells;
        n_entries = n_entries < 0 ? 0 : (n_entries > g.cap_entries ? g.cap_entries : n_entries);
        n_cells = n_cells < 1 ? 1 : (n_cells > g.max_cells ? g.max_cells : n_cells);
        if (e < n_entries) {
            long long lo = 0, hi = n_cells - 1;          // the last cell with cell_start <= e: the entry's own (empty cells share their start with the next)
            while (lo < hi) {
                const long long mid = (lo + hi + 1) >> 1;
                if ((long long)g.cell_start[mid] <= e) lo = mid; else hi = mid - 1;
            }
            home = (int)lo;
            const long long end = g.cell_start[lo + 1];
            t = g.entries[e];
            j0 = e + 1;
            j1 = end < n_entries ? end : n_entries;
        }
    } else if (e < nt) {
        t = e; j0 = e + 1; j1 = nt;
    }
    unsigned long long n_cand = 0, n_hit = 0;
    if (t >= 0 && t < nt && part[t]) {
        MiFace T;
        mi_load(verts, nv, tris, t, T);
        double lo_t[3], hi_t[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) { lo_t[d] = box[6 * t + d]; hi_t[d] = box[6 * t + 3 + d]; }
        for (long long j = j0; j < j1; ++j) {
            const long long u = GRID ? (long long)g.entries[j] : j;
            if (u <= t || u >= nt || !part[u]) continue;             // rows are ascending and without repeats: u <= t only in a grid of another mesh
            const int r = mi_test<IDX, GRID>(verts, nv, tris, box, T, lo_t, hi_t, (int)u, g.head, home);
            if (r == 0) continue;
            ++n_cand;
            if (r != 2) continue;
            ++n_hit;
            if (FILL) {
                const long long at = (long long)row_start[t] + atomicAdd(cursor + t, 1);
                if (at >= 0 && at < n_pairs) { pairs[2 * at] = (int)t; pairs[2 * at + 1] = (int)u; }      // at < n_pairs unless the caller passed another count
            } else atomicAdd(hits + u, 1);
        }
        if (!FILL && n_hit) { atomicAdd(hits + t, (int)n_hit); atomicAdd(first + t, (int)n_hit); }
    }
    if (!FILL) {
        n_cand = wave_sum(n_cand);
        n_hit = wave_sum(n_hit);
        if (lane_id() == 0) {
            if (n_cand) atomicAdd(&tot->n_candidates, n_cand);
            if (n_hit) atomicAdd(&tot->n_pairs, n_hit);
        }
    }
}

// faces in a pair, the most pairs of one face, and the caller's copy of the hits
__global__ __launch_bounds__(256) void k_mi_hits(const int* __restrict__ hits, long long nt, int* __restrict__ face_hits, MiTotals* __restrict__ tot) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int h = t < nt ? hits[t] : 0;
    if (t < nt && face_hits) face_hits[t] = h;
    wave_count(h > 0, &tot->n_faces_hit);
    const unsigned long long m = wave_max((unsigned long long)h);
    if (lane_id() == 0 && m) atomicMax(&tot->max_hits, m);
}

// the eight counts, in the order of mesh_io.INTERSECT_COUNTS
__global__ __launch_bounds__(64) void k_mi_counts(const MiTotals* __restrict__ tot, long long* __restrict__ counts) {
    if (blockIdx.x || threadIdx.x) return;
    counts[0] = (long long)tot->n_bad; counts[1] = (long long)tot->n_nonfinite; counts[2] = (long long)tot->n_faces; counts[3] = (long long)tot->n_skipped;
    counts[4] = (long long)tot->n_candidates; counts[5] = (long long)tot->n_pairs; counts[6] = (long long)tot->n_faces_hit; counts[7] = (long long)tot->max_hits;
}

// one thread per face: the u column of its row of pairs, ascending; rows above ROW_SHORT are listed
__global__ __launch_bounds__(256) void k_mi_rows(const int* __restrict__ first, const int* __restrict__ row_start, long long nt, int* __restrict__ pairs,
                                                 long long n_pairs, int* __restrict__ long_list, MiTotals* __restrict__ tot) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const long long lo = row_start[t], d = first[t];
    if (d < 2 || lo < 0 || lo + d > n_pairs) return;
    if (d > ROW_SHORT) long_list[atomicAdd(&tot->n_long, 1)] = (int)t;
    else row_sort_short<2>(pairs + 2 * lo + 1, (int)d);
}

// one block per listed row: odd-even transposition of the u column in place, d passes
__global__ __launch_bounds__(256) void k_mi_long_rows(const int* __restrict__ first, const int* __restrict__ row_start, int* pairs, const int* __restrict__ long_list,
                                                      const MiTotals* __restrict__ tot) {
    const int n_long = tot->n_long;
    for (int r = blockIdx.x; r < n_long; r += gridDim.x) {
        const int t = long_list[r];
        const int d = first[t];
        int* row = pairs + 2 * (long long)row_start[t] + 1;
        for (int pass = 0; pass < d; ++pass) {
            for (int i = 2 * (int)threadIdx.x + (pass & 1); i + 1 < d; i += 512) {
                const int x = row[2 * i], y = row[2 * i + 2];
                if (x > y) { row[2 * i] = y; row[2 * i + 2] = x; }
            }
            __syncthreads();
        }
    }
}

struct MiCarve {
    MiTotals* tot;
    unsigned char* part;
    double* box;
    int *hits, *first, *row_start, *cursor, *long_list, *block;
    unsigned nb;
};

// the one walk through the workspace: carves it, or sizes it when ws is null; returns its size
static size_t mi_carve(void* ws, long long nv, long long nt, MiCarve& c) {
    (void)nv;                                                        // nothing is kept per vertex
    c.nb = cdiv(nt, SCAN_TILE);
    Carver w(ws);
    c.tot = w.take_bytes<MiTotals>(128);
    c.box = w.take<double>(6 * nt);
    for (int** a : {&c.hits, &c.first, &c.row_start, &c.cursor, &c.long_list}) *a = w.take<int>(nt);
    c.block = w.take<int>(c.nb);
    c.part = w.take<unsigned char>(nt);
    return w.bytes();
}

template <bool FILL>
static void mi_launch_pairs(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, const MdGridView& g, const MiCarve& c, int* pairs,
                            long long n_pairs, hipStream_t s) {
    with_index_type(index_bytes, tris, [&](auto* t) {
        using IDX = index_type<decltype(t)>;
        if (g.head) {
            if (g.cap_entries > 0)
                hipLaunchKernelGGL((k_mi_pairs<IDX, true, FILL>), dim3(cdiv(g.cap_entries, 256)), dim3(256), 0, s, verts, (int)nv, t, nt, c.part, c.box, g, c.hits, c.first,
                                   c.row_start, c.cursor, pairs, n_pairs, c.tot);
        } else
            hipLaunchKernelGGL((k_mi_pairs<IDX, false, FILL>), dim3(cdiv(nt, 256)), dim3(256), 0, s, verts, (int)nv, t, nt, c.part, c.box, g, c.hits, c.first, c.row_start,
                               c.cursor, pairs, n_pairs, c.tot);
    });
}

}  // namespace o2345

using namespace o2345;

extern "C" {

size_t o2345_mesh_intersect_workspace_bytes(long long nv, long long nt) {
    if (!mesh_sizes_ok(nv, nt)) return 0;
    MiCarve c;
    return mi_carve(nullptr, nv, nt, c);
}

// Pass 1: the faces that take part, the search, the per-face hits and the rows of the pair list, all inside the workspace; the eight counts go to
// `counts` on the DEVICE.  No host synchronisation.
int o2345_mesh_intersect_count(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, const void* grid, size_t grid_bytes,
                               long long max_cells, void* workspace, size_t workspace_bytes, long long* counts, int* face_hits_or_null, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_intersect_count", index_bytes);
    O2345_REQUIRE(mesh_sizes_ok(nv, nt), "mesh_intersect_count: bad sizes (nv must stay below 2^30 and 3 * nt below 2^31)");
    O2345_REQUIRE(counts && (nv == 0 || verts) && (nt == 0 || tris), "mesh_intersect_count: null pointer");
    O2345_REQUIRE(((uintptr_t)counts & 7) == 0, "mesh_intersect_count: counts must be 8-byte aligned");
    O2345_REQUIRE_WORKSPACE("mesh_intersect_count", workspace, workspace_bytes, o2345_mesh_intersect_workspace_bytes(nv, nt));
    MdGridView g;
    if (!md_grid_view("mesh_intersect_count", grid, grid_bytes, max_cells, nt, MI_EXHAUSTIVE_MAX, g)) return -1;
    MiCarve c;
    (void)mi_carve(workspace, nv, nt, c);
    hipStream_t s = (hipStream_t)stream;
    O2345_HIP(hipMemsetAsync(c.tot, 0, 128, s));
    if (nt > 0) {
        with_index_type(index_bytes, tris, [&](auto* t) {
            hipLaunchKernelGGL(k_mi_faces<index_type<decltype(t)>>, dim3(cdiv(nt, 256)), dim3(256), 0, s, verts, (int)nv, t, nt, c.part, c.box, c.hits, c.first, c.tot);
        });
        mi_launch_pairs<false>(verts, tris, index_bytes, nv, nt, g, c, nullptr, 0, s);
        exclusive_scan<SCAN_ITEMS>(c.first, nt, c.nb, c.block, c.row_start, nullptr, &c.tot->scan_total, s);
        hipLaunchKernelGGL(k_mi_hits, dim3(cdiv(nt, 256)), dim3(256), 0, s, c.hits, nt, face_hits_or_null, c.tot);
    }
    hipLaunchKernelGGL(k_mi_counts, dim3(1), dim3(64), 0, s, c.tot, counts);
    return check_launch("mesh_intersect_count");
}

// Pass 2: pairs int32 [n_pairs,2] from the workspace of pass 1 (same mesh and grid, untouched in between; n_pairs as counted)
int o2345_mesh_intersect_emit(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, const void* grid, size_t grid_bytes,
                              long long max_cells, void* workspace, long long n_pairs, int* pairs, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_intersect_emit", index_bytes);
    O2345_REQUIRE(mesh_sizes_ok(nv, nt), "mesh_intersect_emit: bad sizes");
    O2345_REQUIRE(n_pairs >= 0 && n_pairs < MI_MAX_PAIRS && (nt > 1 || n_pairs == 0), "mesh_intersect_emit: bad pair count %lld (the limit is 2^30 - 1)", n_pairs);
    O2345_REQUIRE(workspace && (n_pairs == 0 || (pairs && verts && tris)), "mesh_intersect_emit: null pointer");
    O2345_REQUIRE(((uintptr_t)workspace & 15) == 0, "mesh_intersect_emit: workspace must be 16-byte aligned");
    MdGridView g;
    if (!md_grid_view("mesh_intersect_emit", grid, grid_bytes, max_cells, nt, MI_EXHAUSTIVE_MAX, g)) return -1;
    if (n_pairs == 0) return 0;
    MiCarve c;
    (void)mi_carve(workspace, nv, nt, c);
    hipStream_t s = (hipStream_t)stream;
    O2345_HIP(hipMemsetAsync(c.cursor, 0, (size_t)nt * sizeof(int), s));      // a second emit starts over
    O2345_HIP(hipMemsetAsync(&c.tot->n_long, 0, sizeof(int), s));
    mi_launch_pairs<true>(verts, tris, index_bytes, nv, nt, g, c, pairs, n_pairs, s);
    hipLaunchKernelGGL(k_mi_rows, dim3(cdiv(nt, 256)), dim3(256), 0, s, c.first, c.row_start, nt, pairs, n_pairs, c.long_list, c.tot);
    hipLaunchKernelGGL(k_mi_long_rows, dim3(ROW_LONG_GRID), dim3(256), 0, s, c.first, c.row_start, pairs, c.long_list, c.tot);
    return check_launch("mesh_intersect_emit");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_mesh_intersect() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)k_mi_counts);
}
}  // namespace o2345
