// Vertex adjacency of an indexed triangle mesh as a table built on the device, shared by mesh_smooth.hip (the CSR entries and Taubin smoothing) and
// mesh_simplify.hip (every round's neighbour rows).  Equal to the host twin (mesh_io.vertex_adjacency) to the last bit: the table is integer work.
//
// Definitions
//   pairs      every triangle (a, b, c) contributes the ordered pairs (a,b), (b,a), (b,c), (c,b), (c,a), (a,c), minus those with equal ends.
//   row v      the distinct second elements of the pairs whose first element is v, ascending.  The multiplicity of u in row v is the number of such
//              pairs = the number of triangles on edge {u, v}.
//   boundary   boundary[v] = 1 iff some entry of row v has multiplicity exactly 1.  A vertex no triangle references: empty row, boundary 0.
//
// Build: capacities by integer atomicAdd per triangle corner, exclusive scan, slots claimed with an integer atomic cursor (the order inside a raw row is
// arbitrary), then every row is sorted and its duplicates collapsed, which makes the result independent of that order.  Rows of at most ROW_SHORT raw
// entries (marching-cubes meshes: 8 - 24) are sorted by their own thread in registers; longer ones (the centre of a fan) go on a list and get one block
// each, which rank-sorts the row.  No float atomics anywhere.
//
// After adj_build, for every vertex v: rawoff[v] = the start of its row in raw, cap[v] = its degree (row entries raw[rawoff[v] .. + cap[v]), ascending),
// cursor[v] - rawoff[v] = its raw entries (the sum of the multiplicities), bnd[v] = its boundary flag; off[v] = the exclusive scan of the degrees.
// The kernels live in an anonymous namespace: each unit that builds a table instantiates its own copy in its own code object.
#pragma once
#include "mesh_common.h"

namespace o2345 {

// device scalars of one build (workspace head)
struct AdjTotals {
    long long n_raw, n_entries;                     // written by k_scan_small
    unsigned long long n_bad;                       // triangles with an index outside [0, nv)
    int n_long;                                     // rows on the long list
};

namespace {

__global__ __launch_bounds__(256) void k_adj_init(int* __restrict__ cap, int nv, AdjTotals* __restrict__ tot) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v == 0) *tot = AdjTotals{0ll, 0ll, 0ull, 0};
    if (v < nv) cap[v] = 0;
}

// cap[v] = raw entries of row v
template <typename IDX>
__global__ __launch_bounds__(256) void k_adj_capacity(const IDX* __restrict__ tris, long long nt, int nv, int* __restrict__ cap, AdjTotals* __restrict__ tot) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int a, b, c;
    if (!mesh_triangle(tris, t, nv, a, b, c)) { atomicAdd(&tot->n_bad, 1ull); return; }
    const int na = (a != b) + (a != c), nb = (b != a) + (b != c), nc = (c != a) + (c != b);
    if (na) atomicAdd(cap + a, na);
    if (nb) atomicAdd(cap + b, nb);
    if (nc) atomicAdd(cap + c, nc);
}

// every corner claims the slots of its (at most two) pairs with one atomic; cursor[v] starts at the row's first slot and ends behind its last
template <typename IDX>
__global__ __launch_bounds__(256) void k_adj_fill(const IDX* __restrict__ tris, long long nt, int nv, int* __restrict__ cursor, int* __restrict__ raw) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int a, b, c;
    if (!mesh_triangle(tris, t, nv, a, b, c)) return;
    const int na = (a != b) + (a != c), nb = (b != a) + (b != c), nc = (c != a) + (c != b);      // as k_adj_capacity counted them
    if (na) { int s = atomicAdd(cursor + a, na); if (a != b) raw[s++] = b; if (a != c) raw[s] = c; }
    if (nb) { int s = atomicAdd(cursor + b, nb); if (b != c) raw[s++] = c; if (b != a) raw[s] = a; }
    if (nc) { int s = atomicAdd(cursor + c, nc); if (c != a) raw[s++] = a; if (c != b) raw[s] = b; }
}

// a row of at most N raw entries: sorted, duplicates collapsed, written back to the head of its own raw segment -> degree; boundary flag by reference
template <int N>
__device__ __forceinline__ int adj_short_row(int* __restrict__ row, int d, int& boundary) {
    int r[N];
    row_sorted_regs<N>(row, d, r);
    int deg = 0, bnd = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const bool valid = r[k] != ROW_PAD;
        const bool first = k == 0 || r[k] != r[k - 1];
        const bool last = k == N - 1 || r[k] != r[k + 1];
        if (valid && first) {
            row[deg++] = r[k];
            bnd |= last ? 1 : 0;
        }
    }
    boundary = bnd;
    return deg;
}

// one thread per vertex: short rows are finished here (cap[v] becomes the degree), long ones are listed
__global__ __launch_bounds__(256) void k_adj_rows(int nv, const int* __restrict__ rawoff, int* __restrict__ cap, int* __restrict__ raw, unsigned char* __restrict__ bnd,
                                                  int* __restrict__ long_list, AdjTotals* __restrict__ tot) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const int d = cap[v];
    if (d > ROW_SHORT) { long_list[atomicAdd(&tot->n_long, 1)] = (int)v; return; }
    int b = 0, deg = 0;
    if (d > 16) deg = adj_short_row<ROW_SHORT>(raw + rawoff[v], d, b);
    else if (d > 0) deg = adj_short_row<16>(raw + rawoff[v], d, b);
    cap[v] = deg;
    bnd[v] = (unsigned char)b;
}

// one block per listed row: rank sort into tmp (row_rank_sort), then heads of runs compacted back into the row's own raw segment in order
__global__ __launch_bounds__(256) void k_adj_long_rows(const int* __restrict__ rawoff, const int* __restrict__ cursor, int* __restrict__ cap, int* __restrict__ raw,
                                                       int* __restrict__ tmp, unsigned char* __restrict__ bnd, const int* __restrict__ long_list,
                                                       const AdjTotals* __restrict__ tot) {
    __shared__ int lds[5];
    __shared__ int any_single;
    const int n_long = tot->n_long;
    for (int r = blockIdx.x; r < n_long; r += gridDim.x) {
        const int v = long_list[r];
        const int base = rawoff[v], d = cursor[v] - base;
        int* row = raw + base;
        int* srt = tmp + base;
        if (threadIdx.x == 0) any_single = 0;
        row_rank_sort(row, srt, d);                                 // srt complete (this block wrote all of it); row is free from here on
        int run = 0;
        for (int k0 = 0; k0 < d; k0 += 256) {                       // uniform trip count: block_scan_excl synchronises
            const int k = k0 + threadIdx.x;
            const int x = k < d ? srt[k] : ROW_PAD;
            const bool first = k < d && (k == 0 || srt[k - 1] != x);
            const bool last = k < d && (k == d - 1 || srt[k + 1] != x);
            int total;
            const int at = run + block_scan_excl(first ? 1 : 0, lds, total);
            if (first) row[at] = x;
            if (first && last) any_single = 1;
            run += total;
        }
        __syncthreads();
        if (threadIdx.x == 0) { cap[v] = run; bnd[v] = (unsigned char)(any_single ? 1 : 0); }
        __syncthreads();                                            // any_single is reset by the next row
    }
}

}  // namespace

struct AdjCarve {
    AdjTotals* tot;
    int *cap, *rawoff, *cursor, *off, *long_list, *vblock, *raw, *tmp;
    unsigned char* bnd;
    unsigned nbv;
};

// the one walk through the workspace: carves it, or sizes it when ws is null; returns its size.  Everything pass 2 reads lies in front of the one
// nt-sized buffer it needs (raw), so the layout up to there depends on nv alone
inline size_t adj_carve(void* ws, long long nv, long long nt, AdjCarve& c) {
    c.nbv = cdiv(nv, SCAN_TILE);
    Carver w(ws);
    c.tot = w.take_bytes<AdjTotals>(64);
    c.cap = w.take<int>(nv);                        // raw entries per row, then the degree
    c.rawoff = w.take<int>(nv);
    c.cursor = w.take<int>(nv);
    c.off = w.take<int>(nv);                        // exclusive scan of the degrees
    c.long_list = w.take<int>(nv);
    c.vblock = w.take<int>(c.nbv);
    c.bnd = w.take<unsigned char>(nv);
    c.raw = w.take<int>(nt * 6);
    c.tmp = w.take<int>(nt * 6);                    // long rows only
    return w.bytes();
}

static_assert(sizeof(AdjTotals) <= 64, "AdjTotals must fit the workspace head");

inline bool adj_sizes_ok(long long nv, long long nt) { return nv >= 0 && nt >= 0 && nv < (1ll << 30) && nt < (1ll << 31) && 6 * nt < (1ll << 31); }

// the whole build into a carved workspace, queued on s: nothing is read back; offsets = false leaves out the scan of the degrees (off, n_entries)
template <typename IDX>
void adj_build(const IDX* tris, long long nv, long long nt, const AdjCarve& c, hipStream_t s, bool offsets = true) {
    const int n = (int)nv;
    const unsigned gv = cdiv(nv > 0 ? nv : 1, 256), gt = cdiv(nt, 256);
    hipLaunchKernelGGL(k_adj_init, dim3(gv), dim3(256), 0, s, c.cap, n, c.tot);
    // with no vertex every triangle is out of range: the capacity kernel only counts them
    if (nt > 0) hipLaunchKernelGGL(k_adj_capacity<IDX>, dim3(gt), dim3(256), 0, s, tris, nt, n, c.cap, c.tot);
    if (nv > 0) {
        exclusive_scan<SCAN_ITEMS>(c.cap, nv, c.nbv, c.vblock, c.rawoff, c.cursor, &c.tot->n_raw, s);
        if (nt > 0) hipLaunchKernelGGL(k_adj_fill<IDX>, dim3(gt), dim3(256), 0, s, tris, nt, n, c.cursor, c.raw);
        hipLaunchKernelGGL(k_adj_rows, dim3(gv), dim3(256), 0, s, n, c.rawoff, c.cap, c.raw, c.bnd, c.long_list, c.tot);
        if (nt > 0) hipLaunchKernelGGL(k_adj_long_rows, dim3(ROW_LONG_GRID), dim3(256), 0, s, c.rawoff, c.cursor, c.cap, c.raw, c.tmp, c.bnd, c.long_list, c.tot);
        if (offsets) exclusive_scan<SCAN_ITEMS>(c.cap, nv, c.nbv, c.vblock, c.off, nullptr, &c.tot->n_entries, s);
    }
}

}  // namespace o2345
