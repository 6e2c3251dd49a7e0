// Audit of an indexed triangle mesh on the device: is it a closed, oriented 2-manifold, and how good are its triangles.  Read-only; equal to the host
// twin (mesh_io.mesh_audit): integers, flags, per-triangle quality, minima and maxima to the last bit, the three sums to rounding (fixed tree).
//
// Definitions (include/o2345.h has the full text; mesh_audit_math.h the arithmetic)
//   triangle   two equal indices: repeated, counted and flagged, no part in anything else.  The others are the faces: normal, area, volume term, squared
//              edge lengths, quality q = (4 sqrt(3) area) / (l01 + l12 + l20), ten histogram bins.
//   edge       half-edge 3 t + i runs from corner i of face t to corner (i + 1) % 3.  An undirected edge {lo, hi} with m half-edges is a boundary (m = 1),
//              manifold (2) or non-manifold (>= 3) edge; a manifold edge is inconsistent iff both half-edges run the same way, and a consistent one is
//              creased iff both triangles have an area and n . n' < 0.
//   vertex     used, boundary, on a non-manifold edge.  Fans: every manifold edge joins, at each of its two ends, the corners of its two triangles;
//              fans(v) = the classes among the corners at v.  Bow-tie: fans(v) >= 2 and v on no non-manifold edge.
//
// Why thread order does not matter.  Edges: an open-addressing table of 64-bit keys (lo << 32 | hi; atomicCAS, linear probing from dec_mix, at most half
// full).  WHICH slot an edge lands in depends on timing; what the slot holds does not: two integer counts (forward in the low half, backward in the high
// half of one 64-bit atomicAdd) and the smallest and the largest half-edge id (atomicMin / atomicMax) -- for a manifold edge exactly its two half-edges.
// Every half-edge remembers its slot.  A later launch, one thread per triangle, reads the final slots: its own flags and quality without atomics; the
// half-edge that equals its slot's smallest id speaks for the edge (counts, the vertex bits by integer atomicOr, the two fan joins).  Fans: the lock-free
// union-find of mesh_common.h over the 3 nt corners; the classes are the roots (parent[c] == c) once that launch has ended, and every root adds 1 to its
// vertex.  Counts, bounds (as ordered_bits) and sums of the triangle pass: a block folds its 256 triangles into one row of partials, the doubles in a
// fixed tree, and one block folds the rows.  No floating-point atomics; the same bytes on every run.  Inside the inserting kernel every access to the table is an atomic;
// plain loads happen in later launches only.
// Bad input never faults: an index outside [0, nv) is counted and never dereferenced, a vertex with a non-finite coordinate is counted.
#include "mesh_common.h"
#include "mesh_audit_math.h"

namespace o2345 {

constexpr unsigned long long AU_EMPTY = ~0ull;        // no key: lo < hi < 2^30
constexpr unsigned AU_NONE = 0xFFFFFFFFu;             // the slot of a half-edge whose triangle is no face
constexpr int AU_SUMS = 3;                            // area, volume term, quality
constexpr int AU_V_BOUNDARY = 1, AU_V_NONMANIFOLD = 2, AU_V_BOWTIE = 4, AU_V_UNUSED = 8;
constexpr int AU_F_REPEATED = 1, AU_F_ZERO_AREA = 2, AU_F_BOUNDARY = 4, AU_F_NONMANIFOLD = 8, AU_F_INCONSISTENT = 16, AU_F_CREASED = 32;

// one slot of the edge table, 32 bytes: the triangle pass reads a slot with one access, and the four atomics of an insert hit one cache line
struct AuSlot {
    unsigned long long key, counts;                   // lo << 32 | hi; half-edges lo -> hi in the low half, hi -> lo in the high half
    int first, last;                                  // the smallest and the largest half-edge id
    int pad[2];
};
static_assert(sizeof(AuSlot) == 32, "a slot is 32 bytes");

// The triangle pass counts per block, not into the stats block: a wave's atomic on one word runs at some 88 per microsecond, all waves of a launch
// bidding for the same two cache lines made that pass seven times slower than its memory traffic.  Block b writes row b of three tables -- AU_COUNTS
// integers, AU_BOUNDS ordered_bits, AU_SUMS doubles -- and one block folds the rows (k_au_final).  Column k of the integers is word au_entry(k) of the stats.
constexpr int AU_COUNTS = 9 + AU_BINS;                // bad index, repeated, faces, edges, boundary / non-manifold / inconsistent / creased edges, zero area, bins
constexpr int AU_BOUNDS = 3;                          // smallest quality, smallest and largest squared edge length
static_assert(sizeof(O2345AuditStats::histogram) / sizeof(unsigned long long) == AU_BINS, "the stats block holds one entry per bin");
__device__ __forceinline__ int au_entry(int k) {
#define AU_WORD(field) (int)(offsetof(O2345AuditStats, field) / sizeof(unsigned long long))
    constexpr int entry[9] = {AU_WORD(bad_index), AU_WORD(repeated_faces), AU_WORD(faces), AU_WORD(edges), AU_WORD(boundary_edges),
                              AU_WORD(nonmanifold_edges), AU_WORD(inconsistent_edges), AU_WORD(creased_edges), AU_WORD(zero_area_faces)};
    return k < 9 ? entry[k] : AU_WORD(histogram) + (k - 9);
#undef AU_WORD
}

// *counter += the threads of this 256-thread block with pred: one atomic per block (k_au_vertices: a few hundred blocks).  Every thread must call it.
__device__ __forceinline__ void au_block_count(bool pred, int* lds /*[4]*/, unsigned long long* counter) {
    const unsigned long long m = __ballot(pred);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int n = (lds[0] + lds[1]) + (lds[2] + lds[3]);
        if (n) atomicAdd(counter, (unsigned long long)n);
    }
    __syncthreads();
}

__device__ __forceinline__ void au_load(const double* __restrict__ verts, int v, double (&P)[3]) {
    P[0] = verts[3 * (long long)v]; P[1] = verts[3 * (long long)v + 1]; P[2] = verts[3 * (long long)v + 2];
}

// one thread per slot / corner / vertex of whichever array is longest; stats is zero already (a memset in front)
__global__ __launch_bounds__(256) void k_au_init(const double* __restrict__ verts, int nv, AuSlot* __restrict__ slots, long long cap, int* __restrict__ parent, long long nc,
                                                 int* __restrict__ vbits, int* __restrict__ fans, O2345AuditStats* __restrict__ st) {
    __shared__ int lds[4];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < cap) slots[i] = AuSlot{AU_EMPTY, 0ull, 0x7FFFFFFF, -1, {0, 0}};
    if (i < nc) parent[i] = (int)i;
    bool nonfinite = false;
    if (i < nv) {
        vbits[i] = 0; fans[i] = 0;
        nonfinite = !(finite(verts[3 * i]) && finite(verts[3 * i + 1]) && finite(verts[3 * i + 2]));
    }
    if ((long long)blockIdx.x * 256 < nv) au_block_count(nonfinite, lds, &st->nonfinite);       // block-uniform
}

// one thread per triangle: its three half-edges into the table.  The probe is bounded by the capacity; the table is at most half full, so it ends at a
// free slot long before
template <typename IDX>
__global__ __launch_bounds__(256) void k_au_insert(const IDX* __restrict__ tris, long long nt, int nv, AuSlot* slots, unsigned mask, unsigned* __restrict__ hslot) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int v[3];
    const bool face = mesh_triangle(tris, t, nv, v[0], v[1], v[2]) && v[0] != v[1] && v[1] != v[2] && v[0] != v[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const long long h = 3 * t + i;
        unsigned slot = AU_NONE;
        if (face) {
            const int u = v[i], w = v[(i + 1) % 3];
            const unsigned long long key = u < w ? ((unsigned long long)(unsigned)u << 32) | (unsigned)w : ((unsigned long long)(unsigned)w << 32) | (unsigned)u;
            unsigned s = (unsigned)dec_mix(key) & mask;
            for (long long probe = 0; probe <= (long long)mask; ++probe) {
                const unsigned long long prev = atomicCAS(&slots[s].key, AU_EMPTY, key);
                if (prev == AU_EMPTY || prev == key) {
                    atomicAdd(&slots[s].counts, u < w ? 1ull : 1ull << 32);
                    atomicMin(&slots[s].first, (int)h);
                    atomicMax(&slots[s].last, (int)h);
                    slot = s;
                    break;
                }
                s = (s + 1) & mask;
            }
        }
        hslot[h] = slot;
    }
}

// fixed-order sums of AU_SUMS values over a 256-thread block: wave butterflies, then (w0 + w1) + (w2 + w3); valid in thread 0.  The butterfly is written
// out: these are doubles, and its order is part of the result (wave_sum is for integers)
__device__ __forceinline__ void au_block_sums(double (&v)[AU_SUMS]) {
    __shared__ double sm[AU_SUMS][4];
#pragma unroll
    for (int k = 0; k < AU_SUMS; ++k) {
        for (int off = 32; off; off >>= 1) v[k] += __shfl_xor(v[k], off);
        if ((threadIdx.x & 63) == 0) sm[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < AU_SUMS; ++k) v[k] = (sm[k][0] + sm[k][1]) + (sm[k][2] + sm[k][3]);
    }
}

// the block's sum of every integer column (c: the thread's first nine, bin: its histogram bin or -1) and its bounds -> the block's rows; integers and
// minima: any order gives the same result
__device__ __forceinline__ void au_block_row(const int (&c)[9], int bin, unsigned long long q_min, unsigned long long l_min, unsigned long long l_max,
                                             int* __restrict__ row_counts, unsigned long long* __restrict__ row_bounds) {
    __shared__ int sc[4][AU_COUNTS];
    __shared__ unsigned long long sb[4][AU_BOUNDS];
    const int wv = threadIdx.x >> 6;
    const bool first = lane_id() == 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int sum = wave_sum(c[k]);
        if (first) sc[wv][k] = sum;
    }
#pragma unroll
    for (int k = 0; k < AU_BINS; ++k) {
        const int sum = __popcll(__ballot(bin == k));
        if (first) sc[wv][9 + k] = sum;
    }
    q_min = wave_min(q_min); l_min = wave_min(l_min); l_max = wave_max(l_max);
    if (first) { sb[wv][0] = q_min; sb[wv][1] = l_min; sb[wv][2] = l_max; }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < AU_COUNTS) row_counts[k] = (sc[0][k] + sc[1][k]) + (sc[2][k] + sc[3][k]);
    if (k == 0) {
#pragma unroll
        for (int j = 0; j < AU_BOUNDS; ++j) {
            unsigned long long x = sb[0][j];
            for (int w = 1; w < 4; ++w) x = j < 2 ? (sb[w][j] < x ? sb[w][j] : x) : (sb[w][j] > x ? sb[w][j] : x);
            row_bounds[j] = x;
        }
    }
}

// one thread per triangle, after every insert: the triangle's arithmetic, its flags from the final slots of its three half-edges, and for the edges it
// speaks for (its half-edge is the slot's smallest) the counts, the vertex bits and the two fan joins.  Block b -> row b of the partial counts, bounds
// and sums.
template <typename IDX>
__global__ __launch_bounds__(256) void k_au_edges(const double* __restrict__ verts, const IDX* __restrict__ tris, long long nt, int nv,
                                                  const AuSlot* __restrict__ slots, const unsigned* __restrict__ hslot, int* parent, int* vbits, int* __restrict__ counts,
                                                  unsigned long long* __restrict__ bounds, double* __restrict__ partials, unsigned char* __restrict__ face_flags, double* __restrict__ quality) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    double sums[AU_SUMS] = {0.0, 0.0, 0.0};
    unsigned long long q_min = ~0ull, l_min = ~0ull, l_max = 0ull;
    int bin = -1, n_edges = 0, n_boundary = 0, n_nonmanifold = 0, n_inconsistent = 0, n_creased = 0;
    bool zero_area = false, bad = false, repeated = false, face = false;
    if (t < nt) {
        int flags = 0;
        double q = 0.0;
        int v[3];
        const bool in_range = mesh_triangle(tris, t, nv, v[0], v[1], v[2]);
        bad = !in_range;
        repeated = in_range && (v[0] == v[1] || v[1] == v[2] || v[0] == v[2]);
        face = in_range && !repeated;
        if (repeated) flags = AU_F_REPEATED;
        else if (face) {
            double P0[3], P1[3], P2[3];
            au_load(verts, v[0], P0); au_load(verts, v[1], P1); au_load(verts, v[2], P2);
            AuTriangle T;
            au_triangle(P0, P1, P2, T);
            q = T.q;
            zero_area = T.nn == 0.0;
            if (zero_area) flags |= AU_F_ZERO_AREA;
            sums[0] = T.area; sums[1] = T.vol; sums[2] = T.q;
            bin = au_bin(q);
            if (bin >= 0) q_min = ordered_bits(q);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const unsigned long long e = ordered_bits(T.l[k]);
                l_min = e < l_min ? e : l_min;
                l_max = e > l_max ? e : l_max;
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int h = (int)(3 * t + i);
                const unsigned s = hslot[h];
                if (s == AU_NONE) continue;
                const AuSlot e = slots[s];
                const int forward = (int)(e.counts & 0xFFFFFFFFull), m = forward + (int)(e.counts >> 32);
                const int first = e.first, last = e.last;
                const bool speaker = first == h;
                const int u = v[i], w = v[(i + 1) % 3];
                n_edges += speaker;
                if (m == 1) {
                    flags |= AU_F_BOUNDARY;
                    ++n_boundary;
                    atomicOr(vbits + u, AU_V_BOUNDARY); atomicOr(vbits + w, AU_V_BOUNDARY);
                } else if (m >= 3) {
                    flags |= AU_F_NONMANIFOLD;
                    if (speaker) { ++n_nonmanifold; atomicOr(vbits + u, AU_V_NONMANIFOLD); atomicOr(vbits + w, AU_V_NONMANIFOLD); }
                } else {                                             // manifold: first and last are its two half-edges, of two different triangles
                    const int other = speaker ? last : first;
                    const int to = other / 3, j = other - 3 * to;
                    int v2[3];
                    (void)mesh_triangle(tris, to, nv, v2[0], v2[1], v2[2]);      // in the table: a face
                    if (forward != 1) {
                        flags |= AU_F_INCONSISTENT;
                        n_inconsistent += speaker;
                    } else {
                        double Q0[3], Q1[3], Q2[3], n2[3];
                        au_load(verts, v2[0], Q0); au_load(verts, v2[1], Q1); au_load(verts, v2[2], Q2);
                        const double nn2 = au_normal(Q0, Q1, Q2, n2);
                        if (au_creased(T.n, T.nn, n2, nn2)) { flags |= AU_F_CREASED; n_creased += speaker; }
                    }
                    if (speaker) {                                   // the other half-edge starts at u (the same way round) or at w
                        const int j1 = j == 2 ? 0 : j + 1;
                        const bool same = v2[j] == u;
                        cc_union(parent, h, 3 * to + (same ? j : j1));
                        cc_union(parent, (int)(3 * t) + (i + 1) % 3, 3 * to + (same ? j1 : j));
                    }
                }
            }
        }
        if (face_flags) face_flags[t] = (unsigned char)flags;
        if (quality) quality[t] = q;
    }
    const int c[9] = {bad, repeated, face, n_edges, n_boundary, n_nonmanifold, n_inconsistent, n_creased, zero_area};      // the columns of au_entry
    au_block_row(c, bin, q_min, l_min, l_max, counts + (long long)blockIdx.x * AU_COUNTS, bounds + (long long)blockIdx.x * AU_BOUNDS);
    au_block_sums(sums);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < AU_SUMS; ++k) partials[(long long)blockIdx.x * AU_SUMS + k] = sums[k];
    }
}

// one thread per corner, after every join: the classes are the roots, and every root of a face's corner adds 1 to its vertex
template <typename IDX>
__global__ __launch_bounds__(256) void k_au_corners(const IDX* __restrict__ tris, long long nc, const unsigned* __restrict__ hslot, const int* __restrict__ parent,
                                                    int* __restrict__ fans) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= nc || hslot[c] == AU_NONE || parent[c] != (int)c) return;          // a slot: the corner's triangle is a face, its index in range
    atomicAdd(fans + (int)tris[c], 1);
}

// one thread per vertex: classifies, counts, packs the flags
__global__ __launch_bounds__(256) void k_au_vertices(int nv, const int* __restrict__ fans, const int* __restrict__ vbits, unsigned char* __restrict__ vertex_flags,
                                                     O2345AuditStats* __restrict__ st) {
    __shared__ int lds[4];
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    int flags = 0;
    bool used = false;
    if (v < nv) {
        const int f = fans[v];
        flags = vbits[v] & (AU_V_BOUNDARY | AU_V_NONMANIFOLD);
        used = f > 0;
        if (f >= 2 && !(flags & AU_V_NONMANIFOLD)) flags |= AU_V_BOWTIE;
        if (!used) flags |= AU_V_UNUSED;
        if (vertex_flags) vertex_flags[v] = (unsigned char)flags;
    }
    au_block_count(used, lds, &st->vertices);
    au_block_count(flags & AU_V_BOUNDARY, lds, &st->boundary_vertices);
    au_block_count(flags & AU_V_NONMANIFOLD, lds, &st->nonmanifold_vertices);
    au_block_count(flags & AU_V_BOWTIE, lds, &st->bowtie_vertices);
    au_block_count(flags & AU_V_UNUSED, lds, &st->unused_vertices);
}

// one block folds the rows: thread i takes rows i, i + 256, ... in that order, then the block's tree (the doubles: a fixed one); the minima and the
// maximum leave their ordered encoding
__global__ __launch_bounds__(256) void k_au_final(const int* __restrict__ counts, const unsigned long long* __restrict__ bounds, const double* __restrict__ partials,
                                                  long long rows, O2345AuditStats* __restrict__ st) {
    __shared__ unsigned long long sc[4][AU_COUNTS], sb[4][AU_BOUNDS];
    double v[AU_SUMS] = {0.0, 0.0, 0.0};
    unsigned long long c[AU_COUNTS], q_min = ~0ull, l_min = ~0ull, l_max = 0ull;
#pragma unroll
    for (int k = 0; k < AU_COUNTS; ++k) c[k] = 0ull;
    for (long long r = threadIdx.x; r < rows; r += 256) {
#pragma unroll
        for (int k = 0; k < AU_SUMS; ++k) v[k] = v[k] + partials[r * AU_SUMS + k];
#pragma unroll
        for (int k = 0; k < AU_COUNTS; ++k) c[k] += (unsigned long long)counts[r * AU_COUNTS + k];
        const unsigned long long a = bounds[r * AU_BOUNDS], b = bounds[r * AU_BOUNDS + 1], d = bounds[r * AU_BOUNDS + 2];
        q_min = a < q_min ? a : q_min; l_min = b < l_min ? b : l_min; l_max = d > l_max ? d : l_max;
    }
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < AU_COUNTS; ++k) {
        const unsigned long long sum = wave_sum(c[k]);
        if (lane_id() == 0) sc[wv][k] = sum;
    }
    q_min = wave_min(q_min); l_min = wave_min(l_min); l_max = wave_max(l_max);
    if (lane_id() == 0) { sb[wv][0] = q_min; sb[wv][1] = l_min; sb[wv][2] = l_max; }
    au_block_sums(v);                                                // its barrier covers sc and sb
    const int k = threadIdx.x;
    if (k < AU_COUNTS) ((unsigned long long*)st)[au_entry(k)] = (sc[0][k] + sc[1][k]) + (sc[2][k] + sc[3][k]);
    if (k == 0) {
        for (int w = 1; w < 4; ++w) {
            q_min = sb[w][0] < q_min ? sb[w][0] : q_min; l_min = sb[w][1] < l_min ? sb[w][1] : l_min; l_max = sb[w][2] > l_max ? sb[w][2] : l_max;
        }
        st->area = v[0];
        st->volume6 = v[1];
        st->quality_sum = v[2];
        st->quality_min = q_min == ~0ull ? (double)INFINITY : ordered_double(q_min);
        st->edge2_min = l_min == ~0ull ? (double)INFINITY : ordered_double(l_min);
        st->edge2_max = l_max == 0ull ? 0.0 : ordered_double(l_max);
    }
}

struct AuCarve {
    AuSlot* slots;
    int *parent, *vbits, *fans, *counts;
    unsigned long long* bounds;
    unsigned* hslot;
    double* partials;
    long long cap, rows;
};

// the sizes of the adjacency (adj_sizes_ok): vertex indices fit an int, and 6 * nt -- the table's capacity at most -- stays below 2^31
static bool au_sizes_ok(long long nv, long long nt) { return nv >= 0 && nt >= 0 && nv < (1ll << 30) && nt < (1ll << 31) && 6 * nt < (1ll << 31); }

// the one walk through the workspace: carves it, or sizes it when ws is null; returns its size
static size_t au_carve(void* ws, long long nv, long long nt, AuCarve& c) {
    c.cap = 4;                                                       // the power of two >= 6 nt (and >= 4): at most half full
    while (c.cap < 6 * nt) c.cap <<= 1;
    c.rows = (nt + 255) / 256;
    Carver w(ws);
    c.slots = w.take_bytes<AuSlot>((size_t)c.cap * sizeof(AuSlot));
    c.hslot = w.take<unsigned>(3 * nt);
    c.parent = w.take<int>(3 * nt);
    c.vbits = w.take<int>(nv);
    c.fans = w.take<int>(nv);
    c.partials = w.take<double>(c.rows * AU_SUMS);
    c.bounds = w.take<unsigned long long>(c.rows * AU_BOUNDS);
    c.counts = w.take<int>(c.rows * AU_COUNTS);
    return w.bytes();
}

}  // namespace o2345

using namespace o2345;

extern "C" {

size_t o2345_mesh_audit_workspace_bytes(long long nv, long long nt) {
    if (!au_sizes_ok(nv, nt)) return 0;
    AuCarve c;
    return au_carve(nullptr, nv, nt, c);
}

int o2345_mesh_audit(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, void* workspace, size_t workspace_bytes,
                     O2345AuditStats* stats, unsigned char* vertex_flags_or_null, unsigned char* face_flags_or_null, double* quality_or_null, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_audit", index_bytes);
    O2345_REQUIRE(au_sizes_ok(nv, nt), "mesh_audit: bad sizes (nv must stay below 2^30 and 6 * nt below 2^31)");
    O2345_REQUIRE(stats && (nv == 0 || verts) && (nt == 0 || tris), "mesh_audit: null pointer");
    O2345_REQUIRE_WORKSPACE("mesh_audit", workspace, workspace_bytes, o2345_mesh_audit_workspace_bytes(nv, nt));
    O2345_REQUIRE(((uintptr_t)stats & 7) == 0, "mesh_audit: stats must be 8-byte aligned");
    AuCarve c;
    (void)au_carve(workspace, nv, nt, c);
    hipStream_t s = (hipStream_t)stream;
    const int n = (int)nv;
    const long long nc = 3 * nt;
    const long long longest = c.cap > nc ? (c.cap > nv ? c.cap : nv) : (nc > nv ? nc : nv);
    O2345_HIP(hipMemsetAsync(stats, 0, sizeof(O2345AuditStats), s));
    hipLaunchKernelGGL(k_au_init, dim3(cdiv(longest, 256)), dim3(256), 0, s, verts, n, c.slots, c.cap, c.parent, nc, c.vbits, c.fans, stats);
    if (nt > 0) with_index_type(index_bytes, tris, [&](auto* t) {
        using IDX = index_type<decltype(t)>;
        const unsigned gt = cdiv(nt, 256);
        hipLaunchKernelGGL(k_au_insert<IDX>, dim3(gt), dim3(256), 0, s, t, nt, n, c.slots, (unsigned)(c.cap - 1), c.hslot);
        hipLaunchKernelGGL(k_au_edges<IDX>, dim3(gt), dim3(256), 0, s, verts, t, nt, n, c.slots, c.hslot, c.parent, c.vbits, c.counts, c.bounds, c.partials,
                           face_flags_or_null, quality_or_null);
        hipLaunchKernelGGL(k_au_corners<IDX>, dim3(cdiv(nc, 256)), dim3(256), 0, s, t, nc, c.hslot, c.parent, c.fans);
    });
    if (nv > 0) hipLaunchKernelGGL(k_au_vertices, dim3(cdiv(nv, 256)), dim3(256), 0, s, n, c.fans, c.vbits, vertex_flags_or_null, stats);
    hipLaunchKernelGGL(k_au_final, dim3(1), dim3(256), 0, s, c.counts, c.bounds, c.partials, c.rows, stats);
    return check_launch("mesh_audit");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_mesh_audit() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)k_au_final);
}
}  // namespace o2345
