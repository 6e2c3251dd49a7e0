// Hole filling of an indexed triangle mesh on the device: finds the boundary loops and closes them, a loop of three edges with one triangle, a longer
// one with a fan around its centroid.  Equal to the host twin (mesh_io.fill_holes) to the last bit: vertices, triangles, hole numbers and the eight counts.
//
// Definitions (include/o2345.h has the full text)
//   half-edge  3 t + i runs from corner i of triangle t to corner (i + 1) % 3.  A triangle with two equal indices takes no part.  A half-edge is a BOUNDARY
//              half-edge iff its undirected edge {lo, hi} has no other half-edge.
//   next       a vertex is SIMPLE iff exactly one boundary half-edge leaves it and exactly one enters it; next(h) of a boundary half-edge that enters a
//              simple vertex is the one that leaves it, and undefined otherwise.  next is injective: the boundary half-edges fall into cycles -- the HOLES
//              -- and chains, which end at a vertex that is not simple and stay open.
//   hole       leader = its smallest half-edge; rank = the distance from the leader along next; L = its half-edges (>= 3).  Holes are ordered by leader.
//   fill       iff L <= max_edges.  L == 3: the triangle (o_0, o_2, o_1) of the origins in rank order.  L >= 4: a new vertex c = (the sequential fp64 sum
//              of P[o_0] .. P[o_{L-1}]) / L and the triangles (o_{k+1 mod L}, o_k, c): each carries the half-edge opposite to the one it closes.
//
// How.  Boundary half-edges are numbered by an exclusive scan in ascending half-edge order (the COMPACT numbering j: the smallest half-edge of a set is
// its smallest j), next is written in that numbering (-1: undefined).  Two series of pointer-doubling rounds follow, every round one launch that reads
// one buffer of (pointer, value) pairs and writes the other: the first carries the minimum over the path walked so far and ends with pointer -1 exactly
// on the chains; the second runs on the cycles cut open in front of their leader and sums the steps to the end, which gives rank and L.  The number of
// rounds R is the host's: 2^R >= 3 nt bounds every path, whatever the mesh; it is fixed before the first round is launched.  No kernel waits for another
// workgroup or loops until nothing changes; values cross between workgroups at kernel boundaries only, apart from the integer atomics of the edge table
// and of the counters.  Which slot of the table an edge lands in depends on timing; the count the slot ends with does not.  No floating-point atomics:
// one wave per filled hole sums its rim in rank order.  Bad input never faults: a triangle with an index outside [0, nv) is counted and never dereferenced.
#include "mesh_common.h"

namespace o2345 {

constexpr unsigned long long FL_EMPTY = ~0ull;        // no key: lo < hi < 2^30
constexpr unsigned FL_NONE = 0xFFFFFFFFu;             // the slot of a half-edge whose triangle takes no part
constexpr int FL_GRID = 1024;                         // blocks, at most, of the kernels that loop over the boundary half-edges (their number is the device's)

// the head of the workspace: what pass 1 counts, and what pass 2 needs of it
struct FillTotals {
    unsigned long long n_bad, n_overflow, n_open, n_holes, n_too_long, longest;
    long long n_boundary, n_filled, n_new_verts, n_rows;      // the totals of the four scans: rows = the half-edges of the filled holes
    long long max_edges;
};
static_assert(sizeof(FillTotals) <= 128, "FillTotals must fit the workspace head");

// one thread per slot / vertex of whichever array is longer; thread 0 clears the head
__global__ __launch_bounds__(256) void k_fl_init(unsigned long long* __restrict__ keys, int* __restrict__ cnt, long long cap, int* __restrict__ vout, int* __restrict__ vin,
                                                 int* __restrict__ vleave, int nv, long long max_edges, FillTotals* __restrict__ tot) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < cap) { keys[i] = FL_EMPTY; cnt[i] = 0; }
    if (i < nv) { vout[i] = 0; vin[i] = 0; vleave[i] = -1; }
    if (i == 0) {
        *tot = FillTotals{};
        tot->max_edges = max_edges;
    }
}

// one thread per triangle: its three half-edges into the table, one count per undirected edge.  The probe is bounded by the capacity; the table is at
// most half full, so it ends at a free slot long before
template <typename IDX>
__global__ __launch_bounds__(256) void k_fl_insert(const IDX* __restrict__ tris, long long nt, int nv, unsigned long long* keys, int* cnt, unsigned mask,
                                                   unsigned* __restrict__ hslot, FillTotals* tot) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    int v[3] = {0, 0, 0};
    const bool in_range = t < nt && mesh_triangle(tris, t, nv, v[0], v[1], v[2]);
    wave_count(t < nt && !in_range, &tot->n_bad);
    if (t >= nt) return;
    const bool face = in_range && v[0] != v[1] && v[1] != v[2] && v[0] != v[2];
    bool lost = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        unsigned slot = FL_NONE;
        if (face) {
            const int u = v[i], w = v[(i + 1) % 3];
            const unsigned long long key = u < w ? ((unsigned long long)(unsigned)u << 32) | (unsigned)w : ((unsigned long long)(unsigned)w << 32) | (unsigned)u;
            unsigned s = (unsigned)dec_mix(key) & mask;
            for (long long probe = 0; probe <= (long long)mask; ++probe) {
                const unsigned long long prev = atomicCAS(&keys[s], FL_EMPTY, key);
                if (prev == FL_EMPTY || prev == key) {
                    atomicAdd(&cnt[s], 1);
                    slot = s;
                    break;
                }
                s = (s + 1) & mask;
            }
            lost |= slot == FL_NONE;
        }
        hslot[3 * t + i] = slot;
    }
    if (lost) atomicAdd(&tot->n_overflow, 1ull);                      // cannot happen: the table has room for every half-edge
}

// one thread per half-edge, after every insert: flag[h] = boundary, and the boundary half-edges counted at their two ends; a vertex remembers one that
// leaves it (read at simple vertices only: one writer there)
template <typename IDX>
__global__ __launch_bounds__(256) void k_fl_boundary(const IDX* __restrict__ tris, long long nh, const int* __restrict__ cnt, const unsigned* __restrict__ hslot,
                                                     int* __restrict__ flag, int* vout, int* vin, int* __restrict__ vleave) {
    const long long h = (long long)blockIdx.x * 256 + threadIdx.x;
    if (h >= nh) return;
    const unsigned s = hslot[h];
    const bool on = s != FL_NONE && cnt[s] == 1;
    flag[h] = on ? 1 : 0;
    if (!on) return;
    const long long t = h / 3;
    const int i = (int)(h - 3 * t);
    const int u = (int)tris[h], w = (int)tris[3 * t + (i + 1) % 3];       // a slot: the triangle is a face, its indices in range
    atomicAdd(vout + u, 1);
    atomicAdd(vin + w, 1);
    vleave[u] = (int)h;
}

// one thread per half-edge, after the scan: boundary half-edge h becomes j = pos[h]: its id, its origin, next in the compact numbering, and the first
// series' start (pointer = next, value = j)
template <typename IDX>
__global__ __launch_bounds__(256) void k_fl_compact(const IDX* __restrict__ tris, long long nh, const int* __restrict__ flag, const int* __restrict__ pos,
                                                    const int* __restrict__ vout, const int* __restrict__ vin, const int* __restrict__ vleave, int* __restrict__ org,
                                                    int* __restrict__ nxt, int2* __restrict__ pair) {
    const long long h = (long long)blockIdx.x * 256 + threadIdx.x;
    if (h >= nh || !flag[h]) return;
    const long long t = h / 3;
    const int i = (int)(h - 3 * t);
    const int u = (int)tris[h], w = (int)tris[3 * t + (i + 1) % 3];
    const int j = pos[h];
    const int n = vout[w] == 1 && vin[w] == 1 ? pos[vleave[w]] : -1;
    org[j] = u;
    nxt[j] = n;
    pair[j] = make_int2(n, j);
}

// One doubling round over the boundary half-edges, src -> dst: (p, v) of j becomes (p of p, v combined with v of p), or stays when p is -1.  SUM false:
// the smaller value (the smallest half-edge on the path); true: the sum (the steps to the end of a cut cycle).
template <bool SUM>
__global__ __launch_bounds__(256) void k_fl_round(const int2* __restrict__ src, int2* __restrict__ dst, const FillTotals* __restrict__ tot) {
    const long long nb = tot->n_boundary;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < nb; j += (long long)gridDim.x * 256) {
        int2 a = src[j];
        if (a.x >= 0) {
            const int2 b = src[a.x];
            a.y = SUM ? a.y + b.y : (b.y < a.y ? b.y : a.y);
            a.x = b.x;
        }
        dst[j] = a;
    }
}

// between the two series: a pointer that is still alive walks a cycle, and the value is the cycle's leader; lead[j] = that, or -1 on a chain.  The
// second series starts on the cycles cut in front of their leader: (next, 1), and (-1, 0) at the last half-edge and on the chains
__global__ __launch_bounds__(256) void k_fl_cut(const int2* __restrict__ fin, const int* __restrict__ nxt, int* __restrict__ lead, int2* __restrict__ pair,
                                                FillTotals* tot) {
    const long long nb = tot->n_boundary;
    const long long stride = (long long)gridDim.x * 256;
    for (long long j0 = (long long)blockIdx.x * 256; j0 < nb; j0 += stride) {        // block-uniform: every lane reaches wave_count
        const long long j = j0 + threadIdx.x;
        bool open = false;
        if (j < nb) {
            const int2 a = fin[j];
            const bool cycle = a.x >= 0;
            open = !cycle;
            lead[j] = cycle ? a.y : -1;
            const int n = nxt[j];
            pair[j] = cycle && n != a.y ? make_int2(n, 1) : make_int2(-1, 0);
        }
        wave_count(open, &tot->n_open);
    }
}

// one thread per half-edge SLOT (j < nh, zeros behind the boundary half-edges: the scans run over nh entries), after the second series: rank[j], and at
// every leader the hole's length, whether it is filled, and what it adds
__global__ __launch_bounds__(256) void k_fl_holes(const int2* __restrict__ fin, const int* __restrict__ lead, long long nh, int* __restrict__ rank, int* __restrict__ filled,
                                                  int* __restrict__ new_vert, int* __restrict__ rows, FillTotals* tot) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nb = tot->n_boundary;
    bool hole = false, too_long = false;
    int L = 0;
    if (j < nb) {
        const int l = lead[j];
        if (l >= 0) rank[j] = fin[l].y - fin[j].y;                   // steps from the leader = the leader's steps to the end - mine
        hole = l == (int)j;
        if (hole) {
            L = fin[j].y + 1;
            too_long = (long long)L > tot->max_edges;
        }
    }
    if (j < nh) {
        const bool fill = hole && !too_long;
        filled[j] = fill ? 1 : 0;
        new_vert[j] = fill && L >= 4 ? 1 : 0;
        rows[j] = fill ? L : 0;
    }
    wave_count(hole, &tot->n_holes);
    wave_count(too_long, &tot->n_too_long);
    const unsigned long long longest = wave_max((unsigned long long)L);
    if (lane_id() == 0 && longest) atomicMax(&tot->longest, longest);
}

// after the three scans: the origins of every filled hole into its row, in rank order, every row entry with its leader; the filled holes' leaders listed
__global__ __launch_bounds__(256) void k_fl_rows(const int* __restrict__ lead, const int* __restrict__ rank, const int* __restrict__ org, const int* __restrict__ rows,
                                                 const int* __restrict__ row_at, const int* __restrict__ filled_at, int* __restrict__ row, int* __restrict__ row_lead,
                                                 int* __restrict__ hole_list, const FillTotals* __restrict__ tot) {
    const long long nb = tot->n_boundary;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < nb; j += (long long)gridDim.x * 256) {
        const int l = lead[j];
        if (l < 0 || rows[l] == 0) continue;
        const int e = row_at[l] + rank[j];
        row[e] = org[j];
        row_lead[e] = l;
        if (l == (int)j) hole_list[filled_at[l]] = l;
    }
}

// pass 2, one wave per filled hole of four edges or more: the new vertex.  The lanes load 64 rim positions at a time, and every lane adds them in rank
// order, one after the other (-ffp-contract=off and the explicit _rn forms keep it the twin's sum)
__global__ __launch_bounds__(256) void k_fl_centroids(const double* __restrict__ verts, int nv, const int* __restrict__ hole_list, const int* __restrict__ rows,
                                                      const int* __restrict__ row_at, const int* __restrict__ new_vert_at, const int* __restrict__ row,
                                                      const FillTotals* __restrict__ tot, double* __restrict__ verts_out) {
    const long long n_filled = tot->n_filled;
    const int lane = lane_id();
    for (long long k = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); k < n_filled; k += (long long)gridDim.x * 4) {      // wave-uniform
        const int l = hole_list[k], L = rows[l];
        if (L < 4) continue;
        const int lo = row_at[l];
        double ax = 0.0, ay = 0.0, az = 0.0;
        for (int base = 0; base < L; base += 64) {
            double x = 0.0, y = 0.0, z = 0.0;
            if (base + lane < L) {
                const long long u = row[lo + base + lane];
                x = verts[3 * u]; y = verts[3 * u + 1]; z = verts[3 * u + 2];
            }
            const int m = L - base < 64 ? L - base : 64;
            for (int i = 0; i < m; ++i) {
                ax = __dadd_rn(ax, __shfl(x, i));
                ay = __dadd_rn(ay, __shfl(y, i));
                az = __dadd_rn(az, __shfl(z, i));
            }
        }
        if (lane == 0) {
            const long long c = (long long)nv + new_vert_at[l];
            const double n = (double)L;
            verts_out[3 * c] = __ddiv_rn(ax, n); verts_out[3 * c + 1] = __ddiv_rn(ay, n); verts_out[3 * c + 2] = __ddiv_rn(az, n);
        }
    }
}

// pass 2, one thread per row entry: its triangle.  A hole of three edges has one triangle, written by its first entry; its place among the new
// triangles: the row's start less two for every hole of three edges in front (the filled holes in front less those with a new vertex)
template <typename IDX>
__global__ __launch_bounds__(256) void k_fl_tris(int nv, long long nt, const int* __restrict__ rows, const int* __restrict__ row_at, const int* __restrict__ filled_at,
                                                 const int* __restrict__ new_vert_at, const int* __restrict__ row, const int* __restrict__ row_lead,
                                                 const FillTotals* __restrict__ tot, IDX* __restrict__ tris_out, int* __restrict__ hole) {
    const long long n_rows = tot->n_rows;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n_rows; e += (long long)gridDim.x * 256) {
        const int l = row_lead[e], L = rows[l], lo = row_at[l], k = (int)(e - lo);
        const long long at = (long long)lo - 2ll * (filled_at[l] - new_vert_at[l]);
        long long t;
        IDX a, b, c;
        if (L == 3) {
            if (k) continue;
            t = at;
            a = (IDX)row[lo]; b = (IDX)row[lo + 2]; c = (IDX)row[lo + 1];
        } else {
            t = at + k;
            a = (IDX)row[lo + (k + 1 == L ? 0 : k + 1)]; b = (IDX)row[e]; c = (IDX)((long long)nv + new_vert_at[l]);
        }
        if (tris_out) { tris_out[3 * (nt + t)] = a; tris_out[3 * (nt + t) + 1] = b; tris_out[3 * (nt + t) + 2] = c; }
        if (hole) hole[t] = filled_at[l];
    }
}

// the end of pass 1, one thread: the eight counts of the header, in its order.  A hole of three edges has three row entries and one triangle
__global__ __launch_bounds__(64) void k_fl_counts(long long nv, long long nt, const FillTotals* __restrict__ tot, long long* __restrict__ counts) {
    if (threadIdx.x) return;
    counts[0] = tot->n_boundary;
    counts[1] = (long long)tot->n_holes;
    counts[2] = tot->n_filled;
    counts[3] = (long long)tot->n_too_long;
    counts[4] = (long long)tot->n_open;
    counts[5] = (long long)tot->longest;
    counts[6] = nv + tot->n_new_verts;
    counts[7] = nt + tot->n_rows - 2 * (tot->n_filled - tot->n_new_verts);
}

struct FillCarve {
    FillTotals* tot;
    unsigned long long* keys;
    int *cnt, *vout, *vin, *vleave, *flag, *pos, *org, *nxt, *lead, *rank, *new_vert, *rows, *new_vert_at, *row_at, *block;
    int2 *pair_a, *pair_b;
    unsigned* hslot;
    // aliases.  After the compaction flag and pos are free: the filled flags and their scan.  After k_fl_holes the two pair buffers are: the rows, and
    // the list of filled holes
    int *filled, *filled_at, *row, *row_lead, *hole_list;
    long long cap, nh;
    unsigned nbh;
    int rounds;
};

// the one walk through the workspace: carves it, or sizes it when ws is null; returns its size
static size_t fill_carve(void* ws, long long nv, long long nt, FillCarve& c) {
    c.nh = 3 * nt;
    c.cap = 2;                                                       // the power of two >= 2 * the half-edges (and >= 2): at most half full
    while (c.cap < 2 * c.nh) c.cap <<= 1;
    c.rounds = 0;                                                    // 2^rounds >= the half-edges >= any path of boundary half-edges
    while ((1ll << c.rounds) < c.nh) ++c.rounds;
    c.nbh = cdiv(c.nh, SCAN_TILE);
    Carver w(ws);
    c.tot = w.take_bytes<FillTotals>(128);
    c.keys = w.take_bytes<unsigned long long>((size_t)c.cap * sizeof(unsigned long long));      // powers of two, unpadded (16 bytes at the smallest)
    c.cnt = w.take<int>(c.cap);
    c.hslot = w.take<unsigned>(c.nh);
    for (int** a : {&c.vout, &c.vin, &c.vleave}) *a = w.take<int>(nv);
    for (int** a : {&c.flag, &c.pos, &c.org, &c.nxt, &c.lead, &c.rank, &c.new_vert, &c.rows, &c.new_vert_at, &c.row_at}) *a = w.take<int>(c.nh);
    c.pair_a = w.take<int2>(c.nh);
    c.pair_b = w.take<int2>(c.nh);
    c.block = w.take<int>(c.nbh);
    c.filled = c.flag; c.filled_at = c.pos;
    c.row = (int*)c.pair_a; c.row_lead = c.row + c.nh;
    c.hole_list = (int*)c.pair_b;
    return w.bytes();
}

static unsigned fill_grid(long long n) {
    const unsigned g = cdiv(n, 256);
    return g < (unsigned)FL_GRID ? (g ? g : 1u) : (unsigned)FL_GRID;
}

}  // namespace o2345

using namespace o2345;

extern "C" {

size_t o2345_mesh_fill_workspace_bytes(long long nv, long long nt) {
    if (!mesh_sizes_ok(nv, nt)) return 0;
    FillCarve c;
    return fill_carve(nullptr, nv, nt, c);
}

// Pass 1 of the two-call protocol: the boundary, its cycles and chains, the holes' lengths, ranks and rows, all inside the workspace; the eight counts go
// to `counts` on the DEVICE (the caller copies them and allocates the outputs).  Synchronises the stream once, for the refusals that only the device can
// count: they are this call's status.
int o2345_mesh_fill_count(const void* tris, int index_bytes, long long nv, long long nt, long long max_edges, void* workspace, size_t workspace_bytes,
                          long long* counts, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_fill_count", index_bytes);
    O2345_REQUIRE(max_edges >= 3 && max_edges < (1ll << 31), "mesh_fill_count: max_edges must be in [3, 2^31) (a hole has at least three edges), got %lld", max_edges);
    O2345_REQUIRE(mesh_sizes_ok(nv, nt), "mesh_fill_count: bad sizes (nv must stay below 2^30 and 3 * nt below 2^31)");
    O2345_REQUIRE(counts && (nt == 0 || tris), "mesh_fill_count: null pointer");
    O2345_REQUIRE(((uintptr_t)counts & 7) == 0, "mesh_fill_count: counts must be 8-byte aligned");
    O2345_REQUIRE_WORKSPACE("mesh_fill_count", workspace, workspace_bytes, o2345_mesh_fill_workspace_bytes(nv, nt));
    FillCarve c;
    (void)fill_carve(workspace, nv, nt, c);
    hipStream_t s = (hipStream_t)stream;
    const int n = (int)nv;
    const long long nh = c.nh;
    hipLaunchKernelGGL(k_fl_init, dim3(cdiv(c.cap > nv ? c.cap : nv, 256)), dim3(256), 0, s, c.keys, c.cnt, c.cap, c.vout, c.vin, c.vleave, n, max_edges, c.tot);
    if (nt > 0) {
        const unsigned gh = cdiv(nh, 256), gb = fill_grid(nh);
        with_index_type(index_bytes, tris, [&](auto* t) {
            using IDX = index_type<decltype(t)>;
            hipLaunchKernelGGL(k_fl_insert<IDX>, dim3(cdiv(nt, 256)), dim3(256), 0, s, t, nt, n, c.keys, c.cnt, (unsigned)(c.cap - 1), c.hslot, c.tot);
            hipLaunchKernelGGL(k_fl_boundary<IDX>, dim3(gh), dim3(256), 0, s, t, nh, c.cnt, c.hslot, c.flag, c.vout, c.vin, c.vleave);
            exclusive_scan<SCAN_ITEMS>(c.flag, nh, c.nbh, c.block, c.pos, nullptr, &c.tot->n_boundary, s);
            hipLaunchKernelGGL(k_fl_compact<IDX>, dim3(gh), dim3(256), 0, s, t, nh, c.flag, c.pos, c.vout, c.vin, c.vleave, c.org, c.nxt, c.pair_a);
        });
        int2 *src = c.pair_a, *dst = c.pair_b;
        for (int r = 0; r < c.rounds; ++r) {
            hipLaunchKernelGGL(k_fl_round<false>, dim3(gb), dim3(256), 0, s, src, dst, c.tot);
            int2* x = src; src = dst; dst = x;
        }
        hipLaunchKernelGGL(k_fl_cut, dim3(gb), dim3(256), 0, s, src, c.nxt, c.lead, dst, c.tot);
        { int2* x = src; src = dst; dst = x; }
        for (int r = 0; r < c.rounds; ++r) {
            hipLaunchKernelGGL(k_fl_round<true>, dim3(gb), dim3(256), 0, s, src, dst, c.tot);
            int2* x = src; src = dst; dst = x;
        }
        hipLaunchKernelGGL(k_fl_holes, dim3(gh), dim3(256), 0, s, src, c.lead, nh, c.rank, c.filled, c.new_vert, c.rows, c.tot);
        exclusive_scan<SCAN_ITEMS>(c.filled, nh, c.nbh, c.block, c.filled_at, nullptr, &c.tot->n_filled, s);
        exclusive_scan<SCAN_ITEMS>(c.new_vert, nh, c.nbh, c.block, c.new_vert_at, nullptr, &c.tot->n_new_verts, s);
        exclusive_scan<SCAN_ITEMS>(c.rows, nh, c.nbh, c.block, c.row_at, nullptr, &c.tot->n_rows, s);
        hipLaunchKernelGGL(k_fl_rows, dim3(gb), dim3(256), 0, s, c.lead, c.rank, c.org, c.rows, c.row_at, c.filled_at, c.row, c.row_lead, c.hole_list, c.tot);
    }
    hipLaunchKernelGGL(k_fl_counts, dim3(1), dim3(64), 0, s, nv, nt, c.tot, counts);
    int rc = check_launch("mesh_fill_count");
    if (rc) return rc;
    FillTotals h;
    if ((rc = read_totals(h, c.tot, s, "mesh_fill_count"))) return rc;
    O2345_REQUIRE(h.n_bad == 0, "mesh_fill_count: %llu triangles index outside 0 .. %lld", h.n_bad, nv - 1);
    O2345_REQUIRE(h.n_overflow == 0, "mesh_fill_count: %llu probes found no slot (internal error)", h.n_overflow);
    const long long nv_out = nv + h.n_new_verts, nt_out = nt + h.n_rows - 2 * (h.n_filled - h.n_new_verts);      // as k_fl_counts
    O2345_REQUIRE(mesh_sizes_ok(nv_out, nt_out), "mesh_fill_count: bad sizes after the fill (%lld vertices, %lld triangles: nv must stay below 2^30 and 3 * nt below 2^31)",
                  nv_out, nt_out);
    return 0;
}

// Pass 2: verts_out fp64 [nv_out,3], tris_out [nt_out,3] of the input's width, hole int32 [nt_out - nt], from the workspace of pass 1 (same nv and nt,
// untouched in between).  Any output may be NULL.
int o2345_mesh_fill_emit(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, void* workspace, double* verts_out, void* tris_out,
                         int* hole, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_fill_emit", index_bytes);
    O2345_REQUIRE(mesh_sizes_ok(nv, nt), "mesh_fill_emit: bad sizes");
    O2345_REQUIRE(workspace && (!verts_out || verts || nv == 0) && (!tris_out || tris || nt == 0), "mesh_fill_emit: null pointer");
    FillCarve c;
    (void)fill_carve(workspace, nv, nt, c);
    hipStream_t s = (hipStream_t)stream;
    if (verts_out && nv > 0) O2345_HIP(hipMemcpyAsync(verts_out, verts, (size_t)nv * 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (tris_out && nt > 0) O2345_HIP(hipMemcpyAsync(tris_out, tris, (size_t)nt * 3 * (size_t)index_bytes, hipMemcpyDeviceToDevice, s));
    if (nt > 0) {
        const unsigned gb = fill_grid(c.nh);
        if (verts_out)
            hipLaunchKernelGGL(k_fl_centroids, dim3(gb), dim3(256), 0, s, verts, (int)nv, c.hole_list, c.rows, c.row_at, c.new_vert_at, c.row, c.tot, verts_out);
        if (tris_out || hole) with_index_type(index_bytes, tris_out, [&](auto* t) {
            using IDX = index_type<decltype(t)>;
            hipLaunchKernelGGL(k_fl_tris<IDX>, dim3(gb), dim3(256), 0, s, (int)nv, nt, c.rows, c.row_at, c.filled_at, c.new_vert_at, c.row, c.row_lead, c.tot, t, hole);
        });
    }
    return check_launch("mesh_fill_emit");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_mesh_fill() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)k_fl_init);
}
}  // namespace o2345
