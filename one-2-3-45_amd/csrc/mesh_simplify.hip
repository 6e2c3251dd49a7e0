// Simplification of an indexed triangle mesh on the device by rounds of independent half-edge collapses ordered by Garland - Heckbert's quadric error.
// Equal to the host twin (mesh_io.simplify_mesh) to the last bit: integer and topology work, plus the fp64 arithmetic of mesh_simplify_math.h, one
// operation at a time, and sums in a defined order.
//
// Definitions
//   placement  subset placement: collapsing v -> u removes v, u keeps its bits; positions never change.
//   quadrics   once, from the input: K_t = ms_triangle_quadric of triangle t; Q_v = the sequential entrywise sum of K_t over the triangles of v in ascending
//              face order.  After a collapse Q_u <- Q_u + Q_v (Q_u the left operand).
//   round      on its live triangles, N(v) = row v of the adjacency (mesh_adjacency.h).  The half-edge v -> u, u in N(v), is eligible iff (1) every edge at v
//              has exactly two triangles; (2) |N(v) & N(u)| = 2; (3) every triangle at v without u passes ms_keeps_side with P_v replaced by P_u; (4) e =
//              ms_error(Q_v + Q_u, P_u) is finite and cost = (e > 0 ? e : 0) <= max_error.  The candidate of v: its eligible u of least cost, ties to the
//              smaller u.  C candidates, need = ceil((live - target) / 2), bin = ms_bin(cost); B = the smallest bin whose cumulative count reaches
//              max(1, min(8 need, ceil(C / 2))); the candidates with bin <= B take part, priority (dec_mix(v + (round << 32)), v).
//   selection  m1[y] = the smallest priority over y and N(y), m2[v] = the smallest m1 over v and N(v); v is selected iff m2[v] is v's own: the closed
//              1-rings of the selected vertices are disjoint, so all selected collapses apply at once.  Triangles are remapped, those with two equal
//              corners dropped (a dead triangle is stored as (0, 0, 0): it contributes to no table); face order, corner order and orientation stay.
//   stop       live <= target ("target"), no candidate ("blocked"), max_rounds rounds done ("rounds").
//   output     a vertex is kept iff a live triangle references it, in the old order, bit for bit; triangles renumbered by an exclusive scan; source new ->
//              old; merged[v] = the new index of the vertex v ended in, following the collapses, or -1.
//
// Why thread order does not matter.  The adjacency rows are sorted.  The incident-triangle rows are filled through an integer atomic cursor in any order;
// round 0 sorts them before the one sum whose order matters (Q_v), later rounds only AND a test over them.  Row (1): a vertex with k live triangles has
// 2 k raw neighbour entries; no multiplicity 1 (boundary flag 0) and k distinct neighbours make every multiplicity 2.  The histogram, the counts and the
// largest cost are integer atomics whose result does not depend on their order; the two gathers and the selection use none.  The selected collapses of a
// round touch disjoint vertices, so Q_u <- Q_u + Q_v has one writer.  No float atomics anywhere.
#include "mesh_adjacency.h"
#include "mesh_simplify_math.h"

namespace o2345 {

constexpr int SIM_BINS = 2048;                      // the biased exponent field of a double
constexpr int SIM_WIDE = 8, SIM_SHARE = 2;          // the participation rule (mesh_io.SIMPLIFY_WIDE / SIMPLIFY_SHARE)
constexpr unsigned long long SIM_NONE = ~0ull;      // the hash part of "takes no part"; its vertex part is ROW_PAD

// device scalars of one call (workspace head)
struct SimTotals {
    unsigned long long n_nonfinite, n_bad, n_repeated;               // of the input; counted once
    unsigned long long n_candidates, n_selected;                     // of the round
    long long nv_out, nt_out;                                        // written by k_scan_small
    int bin, n_long;                                                 // B of the round; long triangle rows (round 0)
};

__device__ __forceinline__ void sim_point(const double* __restrict__ verts, int v, double (&P)[3]) {
    P[0] = verts[3 * (long long)v]; P[1] = verts[3 * (long long)v + 1]; P[2] = verts[3 * (long long)v + 2];
}

// priority of x in this round: (hash, x) for a participant, (SIM_NONE, ROW_PAD) otherwise
__device__ __forceinline__ void sim_priority(int x, const int* __restrict__ cand, const double* __restrict__ cost, int B, unsigned long long salt,
                                             unsigned long long& h, int& who) {
    const bool part = cand[x] >= 0 && ms_bin(cost[x]) <= B;
    h = part ? dec_mix((unsigned long long)x + salt) : SIM_NONE;
    who = part ? x : ROW_PAD;
}

__device__ __forceinline__ void sim_take_min(unsigned long long h, int who, unsigned long long& bh, int& bw) {
    if (h < bh || (h == bh && who < bw)) { bh = h; bw = who; }
}

// the input -> the working triangles (int, a bad or repeated triangle dead) and the counts of what is refused; parent[v] = v
template <typename IDX>
__global__ __launch_bounds__(256) void k_sim_begin(const double* __restrict__ verts, const IDX* __restrict__ tris, long long nt, int nv, int* __restrict__ cur,
                                                   int* __restrict__ parent, SimTotals* __restrict__ tot) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false, repeated = false, live = false, nonfinite = false;
    if (i < nt) {
        int a, b, c;
        bad = !mesh_triangle(tris, i, nv, a, b, c);
        repeated = !bad && (a == b || b == c || a == c);
        live = !bad && !repeated;
        cur[3 * i] = live ? a : 0; cur[3 * i + 1] = live ? b : 0; cur[3 * i + 2] = live ? c : 0;
    }
    if (i < nv) {
        parent[i] = (int)i;
#pragma unroll
        for (int d = 0; d < 3; ++d) nonfinite |= !finite(verts[3 * i + d]);
    }
    wave_count(bad, &tot->n_bad);
    wave_count(repeated, &tot->n_repeated);
    wave_count(nonfinite, &tot->n_nonfinite);
}

// what a round counts from zero; one thread per vertex, at least SIM_BINS threads
__global__ __launch_bounds__(256) void k_sim_round_init(int nv, int* __restrict__ tfill, int* __restrict__ hist, SimTotals* __restrict__ tot) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) { tot->n_candidates = 0; tot->n_selected = 0; tot->bin = -1; tot->n_long = 0; }
    if (i < SIM_BINS) hist[i] = 0;
    if (i < nv) tfill[i] = 0;
}

// row v of the incident-triangle table starts at rawoff[v] / 2 (a vertex with k live triangles has 2 k raw neighbour entries); the order inside is arbitrary
__global__ __launch_bounds__(256) void k_sim_tfill(const int* __restrict__ cur, long long nt, const int* __restrict__ rawoff, int* __restrict__ tfill,
                                                   int* __restrict__ trow) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int a = cur[3 * t], b = cur[3 * t + 1], c = cur[3 * t + 2];
    if (a == b) return;                                             // dead
    trow[(rawoff[a] >> 1) + atomicAdd(tfill + a, 1)] = (int)t;
    trow[(rawoff[b] >> 1) + atomicAdd(tfill + b, 1)] = (int)t;
    trow[(rawoff[c] >> 1) + atomicAdd(tfill + c, 1)] = (int)t;
}

// Q[v] = acc over row[0 .. k) in the order given: acc = 0; acc = acc + K_t
__device__ __forceinline__ void sim_sum_quadrics(const double* __restrict__ verts, const int* __restrict__ cur, const int* row, int k, double* __restrict__ q) {
    double acc[MS_Q];
#pragma unroll
    for (int i = 0; i < MS_Q; ++i) acc[i] = 0.0;
    for (int j = 0; j < k; ++j) {
        const long long t = row[j];
        double P0[3], P1[3], P2[3], K[MS_Q];
        sim_point(verts, cur[3 * t], P0); sim_point(verts, cur[3 * t + 1], P1); sim_point(verts, cur[3 * t + 2], P2);
        ms_triangle_quadric(P0, P1, P2, K);
#pragma unroll
        for (int i = 0; i < MS_Q; ++i) acc[i] = __dadd_rn(acc[i], K[i]);
    }
#pragma unroll
    for (int i = 0; i < MS_Q; ++i) q[i] = acc[i];
}

// round 0, one thread per vertex: rows of at most ROW_SHORT triangles are sorted here and summed, longer ones are listed
__global__ __launch_bounds__(256) void k_sim_quadrics(const double* __restrict__ verts, int nv, const int* __restrict__ cur, const int* __restrict__ rawoff,
                                                      const int* __restrict__ tfill, int* __restrict__ trow, double* __restrict__ Q, int* __restrict__ long_list,
                                                      SimTotals* __restrict__ tot) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const int k = tfill[v];
    if (k > ROW_SHORT) { long_list[atomicAdd(&tot->n_long, 1)] = (int)v; return; }
    int* row = trow + (rawoff[v] >> 1);
    if (k > 1) row_sort_short(row, k);
    sim_sum_quadrics(verts, cur, row, k, Q + MS_Q * v);
}

// one block per listed row (row_sort_long); thread 0 adds in row order, reading the sorted row where the block has it complete: tmp
__global__ __launch_bounds__(256) void k_sim_quadrics_long(const double* __restrict__ verts, const int* __restrict__ cur, const int* __restrict__ rawoff,
                                                           const int* __restrict__ tfill, int* __restrict__ trow, int* __restrict__ tmp, double* __restrict__ Q,
                                                           const int* __restrict__ long_list, const SimTotals* __restrict__ tot) {
    const int n_long = tot->n_long;
    for (int r = blockIdx.x; r < n_long; r += gridDim.x) {
        const int v = long_list[r];
        const int base = rawoff[v] >> 1, k = tfill[v];
        row_sort_long(trow + base, tmp + base, k);
        if (threadIdx.x == 0) sim_sum_quadrics(verts, cur, tmp + base, k, Q + MS_Q * (long long)v);
    }
}

// one thread per vertex: its candidate (cand[v] = u or -1, cost[v]), the histogram of the candidates' bins and their number
__global__ __launch_bounds__(256) void k_sim_candidate(const double* __restrict__ verts, int nv, const int* __restrict__ cur, const int* __restrict__ rawoff,
                                                       const int* __restrict__ deg, const int* __restrict__ cursor, const unsigned char* __restrict__ bnd,
                                                       const int* __restrict__ raw, const int* __restrict__ trow, const double* __restrict__ Q, double max_error,
                                                       int* __restrict__ cand, double* __restrict__ cost, int* __restrict__ hist, SimTotals* __restrict__ tot) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    int best_u = -1;
    double best_c = 0.0;
    if (v < nv) {
        const int base = rawoff[v], d = deg[v], k = (cursor[v] - base) >> 1;
        if (d > 0 && !bnd[v] && k == d) {                           // (1): every edge at v has exactly two triangles
            double Qv[MS_Q];
#pragma unroll
            for (int i = 0; i < MS_Q; ++i) Qv[i] = Q[MS_Q * v + i];
            const int* tv = trow + (base >> 1);
            for (int n = 0; n < d; ++n) {
                const int u = raw[base + n];
                // (4) first: it is the cheapest test, and a neighbour that cannot win (u ascends: a tie keeps the smaller u) needs no other
                double Pu[3], q[MS_Q];
                sim_point(verts, u, Pu);
#pragma unroll
                for (int i = 0; i < MS_Q; ++i) q[i] = __dadd_rn(Qv[i], Q[MS_Q * (long long)u + i]);
                const double e = ms_error(q, Pu);
                if (!finite(e)) continue;
                const double c = e > 0.0 ? e : 0.0;
                if (!(c <= max_error) || (best_u >= 0 && !(c < best_c))) continue;
                // (2): the entries the two ascending rows share
                const int ub = rawoff[u], ud = deg[u];
                int i1 = 0, i2 = 0, common = 0;
                while (i1 < d && i2 < ud) {
                    const int x = raw[base + i1], y = raw[ub + i2];
                    common += x == y ? 1 : 0;
                    i1 += x <= y ? 1 : 0;
                    i2 += y <= x ? 1 : 0;
                }
                if (common != 2) continue;
                // (3): the triangles at v without u keep their side
                bool ok = true;
                for (int j = 0; j < k && ok; ++j) {
                    const long long t = tv[j];
                    const int a = cur[3 * t], b = cur[3 * t + 1], c3 = cur[3 * t + 2];
                    if (a == u || b == u || c3 == u) continue;
                    double P0[3], P1[3], P2[3];
                    sim_point(verts, a, P0); sim_point(verts, b, P1); sim_point(verts, c3, P2);
                    ok = ms_keeps_side(P0, P1, P2, a == (int)v ? 0 : (b == (int)v ? 1 : 2), Pu);
                }
                if (!ok) continue;
                best_u = u; best_c = c;
            }
        }
        cand[v] = best_u;
        cost[v] = best_c;
        if (best_u >= 0) atomicAdd(hist + ms_bin(best_c), 1);
    }
    wave_count(best_u >= 0, &tot->n_candidates);
}

// one block: B = the smallest bin whose cumulative count reaches max(1, min(SIM_WIDE need, ceil(C / SIM_SHARE))); stays -1 without a candidate
__global__ __launch_bounds__(256) void k_sim_threshold(const int* __restrict__ hist, long long need, SimTotals* __restrict__ tot) {
    __shared__ int lds[5];
    const long long C = (long long)tot->n_candidates;
    long long want = (C + SIM_SHARE - 1) / SIM_SHARE;
    if (SIM_WIDE * need < want) want = SIM_WIDE * need;
    if (want < 1) want = 1;
    constexpr int PER = SIM_BINS / 256;
    int h[PER], s = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { h[j] = hist[PER * threadIdx.x + j]; s += h[j]; }
    int total;
    long long run = block_scan_excl(s, lds, total);
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const long long before = run;
        run += h[j];
        if (before < want && run >= want) tot->bin = PER * threadIdx.x + j;
    }
}

// m1[y] = the smallest priority over y and its row
__global__ __launch_bounds__(256) void k_sim_gather1(int nv, const int* __restrict__ rawoff, const int* __restrict__ deg, const int* __restrict__ raw,
                                                     const int* __restrict__ cand, const double* __restrict__ cost, const SimTotals* __restrict__ tot,
                                                     unsigned long long salt, unsigned long long* __restrict__ m1h, int* __restrict__ m1v) {
    const long long y = (long long)blockIdx.x * 256 + threadIdx.x;
    if (y >= nv) return;
    const int B = tot->bin;
    unsigned long long bh, h;
    int bw, who;
    sim_priority((int)y, cand, cost, B, salt, bh, bw);
    const int base = rawoff[y], d = deg[y];
    for (int n = 0; n < d; ++n) {
        sim_priority(raw[base + n], cand, cost, B, salt, h, who);
        sim_take_min(h, who, bh, bw);
    }
    m1h[y] = bh; m1v[y] = bw;
}

// m2[v] over v and its row; v is selected iff it is v's own priority.  target[v] = the vertex v collapses into, or -1.  A selected v hands its quadric
// to its target (one writer: the closed 1-rings of the selected vertices are disjoint) and counts: this round's entry of the stats, the largest cost
__global__ __launch_bounds__(256) void k_sim_select(int nv, const int* __restrict__ rawoff, const int* __restrict__ deg, const int* __restrict__ raw,
                                                    const int* __restrict__ cand, const double* __restrict__ cost, const unsigned long long* __restrict__ m1h,
                                                    const int* __restrict__ m1v, int* __restrict__ target, int* __restrict__ parent, double* __restrict__ Q,
                                                    SimTotals* __restrict__ tot, unsigned long long* __restrict__ n_round, unsigned long long* __restrict__ max_cost_bits) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    bool selected = false;
    if (v < nv) {
        const int u = cand[v];
        if (u >= 0 && ms_bin(cost[v]) <= tot->bin) {
            unsigned long long bh = m1h[v];
            int bw = m1v[v];
            const int base = rawoff[v], d = deg[v];
            for (int n = 0; n < d; ++n) { const int y = raw[base + n]; sim_take_min(m1h[y], m1v[y], bh, bw); }
            selected = bw == (int)v;
        }
        target[v] = selected ? u : -1;
        if (selected) {
            parent[v] = u;
#pragma unroll
            for (int i = 0; i < MS_Q; ++i) Q[MS_Q * (long long)u + i] = __dadd_rn(Q[MS_Q * (long long)u + i], Q[MS_Q * v + i]);
            atomicMax(max_cost_bits, (unsigned long long)__double_as_longlong(cost[v]));          // costs are >= +0: their bit patterns order like they do
        }
    }
    wave_count(selected, &tot->n_selected);
    wave_count(selected, n_round);
}

// every live triangle through the round's targets; two equal corners: dead.  Exactly two triangles die per collapse (the two on edge {v, u}: every edge
// at v has two, and no triangle holds two selected vertices), which is how the host counts the live ones
__global__ __launch_bounds__(256) void k_sim_apply(int* __restrict__ cur, long long nt, const int* __restrict__ target) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int a = cur[3 * t], b = cur[3 * t + 1], c = cur[3 * t + 2];
    if (a == b) return;                                             // dead
    const int ta = target[a], tb = target[b], tc = target[c];
    if (ta < 0 && tb < 0 && tc < 0) return;
    a = ta >= 0 ? ta : a; b = tb >= 0 ? tb : b; c = tc >= 0 ? tc : c;
    const bool live = a != b && b != c && a != c;
    cur[3 * t] = live ? a : 0; cur[3 * t + 1] = live ? b : 0; cur[3 * t + 2] = live ? c : 0;
}

// tkeep[t] = 1 iff t is alive; the live triangles flag their vertices (every writer stores the same 1)
__global__ __launch_bounds__(256) void k_sim_keep(const int* __restrict__ cur, long long nt, int* __restrict__ tkeep, int* __restrict__ flag) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int a = cur[3 * t], b = cur[3 * t + 1], c = cur[3 * t + 2];
    tkeep[t] = a != b ? 1 : 0;
    if (a != b) { flag[a] = 1; flag[b] = 1; flag[c] = 1; }
}

// the head of the stats block: what the host loop knows, and the two sizes
__global__ void k_sim_finish(const SimTotals* __restrict__ tot, long long rounds, long long stopped, O2345SimplifyStats* __restrict__ stats) {
    stats->rounds = rounds;
    stats->stopped = stopped;
    stats->vertices = tot->nv_out;
    stats->triangles = tot->nt_out;
}

// the collapses of every round, behind the struct in the same buffer (include/o2345.h); the round's kernel counts with an unsigned atomic
static inline unsigned long long* sim_collapses(O2345SimplifyStats* stats) { return (unsigned long long*)(stats + 1); }

// thread v: merged[v] (the end of v's chain of collapses, renumbered, or -1), and the copy of a kept v
__global__ __launch_bounds__(256) void k_sim_emit_verts(const double* __restrict__ verts, int nv, const int* __restrict__ parent, const int* __restrict__ flag,
                                                        const int* __restrict__ vmap, double* __restrict__ verts_out, int* __restrict__ source,
                                                        int* __restrict__ merged) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    if (merged) {
        int r = (int)v;
        for (int i = 0; i < nv && parent[r] != r; ++i) r = parent[r];          // a chain has at most one link per round
        merged[v] = flag[r] ? vmap[r] : -1;
    }
    if (!flag[v]) return;
    const long long o = vmap[v];
    if (verts_out) { verts_out[3 * o] = verts[3 * v]; verts_out[3 * o + 1] = verts[3 * v + 1]; verts_out[3 * o + 2] = verts[3 * v + 2]; }
    if (source) source[o] = (int)v;
}

struct SimCarve {
    SimTotals* tot;
    double *Q, *cost;
    unsigned long long* m1h;
    int *cur, *parent, *tfill, *trow, *long_list, *cand, *m1v, *target, *hist, *flag, *vmap, *tkeep, *tmap, *vblock, *tblock;
    AdjCarve adj;
    unsigned nbv, nbt;
};

static_assert(sizeof(SimTotals) <= 128, "SimTotals must fit the workspace head");

static bool sim_sizes_ok(long long nv, long long nt) { return adj_sizes_ok(nv, nt); }

// the one walk through the workspace: carves it, or sizes it when ws is null; returns its size (bounded by nv and nt alone: the rows total 6 nt entries)
static size_t sim_carve(void* ws, long long nv, long long nt, SimCarve& c) {
    c.nbv = cdiv(nv, SCAN_TILE); c.nbt = cdiv(nt, SCAN_TILE);
    Carver w(ws);
    c.tot = w.take_bytes<SimTotals>(128);
    c.Q = w.take<double>(MS_Q * nv);
    c.cost = w.take<double>(nv);
    c.m1h = w.take<unsigned long long>(nv);
    c.cur = w.take<int>(3 * nt);
    c.trow = w.take<int>(3 * nt);
    for (int** a : {&c.parent, &c.tfill, &c.long_list, &c.cand, &c.m1v, &c.target, &c.flag, &c.vmap}) *a = w.take<int>(nv);
    for (int** a : {&c.tkeep, &c.tmap}) *a = w.take<int>(nt);
    c.hist = w.take<int>(SIM_BINS);
    c.vblock = w.take<int>(c.nbv);
    c.tblock = w.take<int>(c.nbt);
    const size_t head = w.bytes();                                  // a multiple of 16: the adjacency's own walk starts here
    return head + adj_carve(ws ? (char*)ws + head : nullptr, nv, nt, c.adj);
}

}  // namespace o2345

using namespace o2345;

extern "C" {

size_t o2345_mesh_simplify_workspace_bytes(long long nv, long long nt) {
    if (!sim_sizes_ok(nv, nt)) return 0;
    SimCarve c;
    return sim_carve(nullptr, nv, nt, c);
}

// Pass 1 of the two-call protocol: all rounds, the kept flags and the renumbering inside the workspace, the stats block on the device.  Synchronises the
// stream once after the input check and once per round (the host loop needs the round's counts to decide whether another one runs).
int o2345_mesh_simplify_count(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, long long target_faces, double max_error,
                              int max_rounds, void* workspace, size_t workspace_bytes, O2345SimplifyStats* stats, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_simplify_count", index_bytes);
    O2345_REQUIRE(sim_sizes_ok(nv, nt), "mesh_simplify_count: bad sizes (nv must stay below 2^30 and 6 * nt below 2^31)");
    O2345_REQUIRE(target_faces >= 0 && max_rounds >= 0, "mesh_simplify_count: target_faces and max_rounds must be >= 0, got %lld, %d", target_faces, max_rounds);
    O2345_REQUIRE(max_error >= 0.0, "mesh_simplify_count: max_error must be >= 0 (infinity = no limit), got %g", max_error);
    O2345_REQUIRE(workspace && stats && (nv == 0 || verts) && (nt == 0 || tris), "mesh_simplify_count: null pointer");
    O2345_REQUIRE(workspace_bytes >= o2345_mesh_simplify_workspace_bytes(nv, nt), "mesh_simplify_count: workspace too small");
    O2345_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)stats & 7) == 0, "mesh_simplify_count: workspace must be 16-byte aligned, stats 8-byte aligned");
    SimCarve c;
    (void)sim_carve(workspace, nv, nt, c);
    hipStream_t s = (hipStream_t)stream;
    const int n = (int)nv;
    const unsigned gv = cdiv(nv, 256), gt = cdiv(nt, 256);
    O2345_HIP(hipMemsetAsync(c.tot, 0, sizeof(SimTotals), s));
    O2345_HIP(hipMemsetAsync(stats, 0, (size_t)((char*)(sim_collapses(stats) + max_rounds) - (char*)stats), s));      // the struct and collapses[max_rounds]
    if (nv > 0) O2345_HIP(hipMemsetAsync(c.flag, 0, sizeof(int) * (size_t)nv, s));
    if (nv > 0 || nt > 0) with_index_type(index_bytes, tris, [&](auto* t) {
        hipLaunchKernelGGL(k_sim_begin<index_type<decltype(t)>>, dim3(cdiv(nv > nt ? nv : nt, 256)), dim3(256), 0, s, verts, t, nt, n, c.cur, c.parent, c.tot);
    });
    int rc = check_launch("mesh_simplify_count");
    if (rc) return rc;
    SimTotals h;
    if ((rc = read_totals(h, c.tot, s, "mesh_simplify_count"))) return rc;
    O2345_REQUIRE(h.n_nonfinite == 0, "mesh_simplify_count: %llu vertices have a non-finite coordinate", h.n_nonfinite);
    O2345_REQUIRE(h.n_bad == 0, "mesh_simplify_count: %llu triangles index outside 0 .. %lld", h.n_bad, nv - 1);
    O2345_REQUIRE(h.n_repeated == 0, "mesh_simplify_count: %llu triangles repeat a vertex index", h.n_repeated);
    long long live = nt, stopped;                                   // every triangle of a mesh that passed the check is alive
    int round = 0;
    for (;; ++round) {
        if (live <= target_faces) { stopped = O2345_SIMPLIFY_STOPPED_TARGET; break; }
        if (round == max_rounds) { stopped = O2345_SIMPLIFY_STOPPED_ROUNDS; break; }
        const unsigned long long salt = (unsigned long long)round << 32;
        hipLaunchKernelGGL(k_sim_round_init, dim3(cdiv(nv > SIM_BINS ? nv : SIM_BINS, 256)), dim3(256), 0, s, n, c.tfill, c.hist, c.tot);
        adj_build<int>(c.cur, nv, nt, c.adj, s, false);
        hipLaunchKernelGGL(k_sim_tfill, dim3(gt), dim3(256), 0, s, c.cur, nt, c.adj.rawoff, c.tfill, c.trow);
        if (round == 0) {
            hipLaunchKernelGGL(k_sim_quadrics, dim3(gv), dim3(256), 0, s, verts, n, c.cur, c.adj.rawoff, c.tfill, c.trow, c.Q, c.long_list, c.tot);
            hipLaunchKernelGGL(k_sim_quadrics_long, dim3(ROW_LONG_GRID), dim3(256), 0, s, verts, c.cur, c.adj.rawoff, c.tfill, c.trow, c.adj.tmp, c.Q, c.long_list, c.tot);
        }
        hipLaunchKernelGGL(k_sim_candidate, dim3(gv), dim3(256), 0, s, verts, n, c.cur, c.adj.rawoff, c.adj.cap, c.adj.cursor, c.adj.bnd, c.adj.raw, c.trow, c.Q,
                           max_error, c.cand, c.cost, c.hist, c.tot);
        hipLaunchKernelGGL(k_sim_threshold, dim3(1), dim3(256), 0, s, c.hist, (live - target_faces + 1) / 2, c.tot);
        hipLaunchKernelGGL(k_sim_gather1, dim3(gv), dim3(256), 0, s, n, c.adj.rawoff, c.adj.cap, c.adj.raw, c.cand, c.cost, c.tot, salt, c.m1h, c.m1v);
        hipLaunchKernelGGL(k_sim_select, dim3(gv), dim3(256), 0, s, n, c.adj.rawoff, c.adj.cap, c.adj.raw, c.cand, c.cost, c.m1h, c.m1v, c.target, c.parent, c.Q, c.tot,
                           sim_collapses(stats) + round, &stats->max_cost_bits);
        hipLaunchKernelGGL(k_sim_apply, dim3(gt), dim3(256), 0, s, c.cur, nt, c.target);
        if ((rc = check_launch("mesh_simplify_count"))) return rc;
        if ((rc = read_totals(h, c.tot, s, "mesh_simplify_count"))) return rc;
        if (h.n_candidates == 0) { stopped = O2345_SIMPLIFY_STOPPED_BLOCKED; break; }          // nobody took part: nothing was applied
        live -= 2 * (long long)h.n_selected;
    }
    if (nt > 0) {
        hipLaunchKernelGGL(k_sim_keep, dim3(gt), dim3(256), 0, s, c.cur, nt, c.tkeep, c.flag);
        exclusive_scan<SCAN_ITEMS>(c.tkeep, nt, c.nbt, c.tblock, c.tmap, nullptr, &c.tot->nt_out, s);
    }
    if (nv > 0) exclusive_scan<SCAN_ITEMS>(c.flag, nv, c.nbv, c.vblock, c.vmap, nullptr, &c.tot->nv_out, s);
    hipLaunchKernelGGL(k_sim_finish, dim3(1), dim3(1), 0, s, c.tot, (long long)round, stopped, stats);
    return check_launch("mesh_simplify_count");
}

// Pass 2: verts_out fp64 [nv_out,3], tris_out [nt_out,3] of width index_bytes, source int32 [nv_out], merged int32 [nv], from the workspace of pass 1
// (same nv and nt, untouched in between).  Any output may be NULL.
int o2345_mesh_simplify_emit(const double* verts, int index_bytes, long long nv, long long nt, void* workspace, double* verts_out, void* tris_out, int* source,
                             int* merged, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_simplify_emit", index_bytes);
    O2345_REQUIRE(sim_sizes_ok(nv, nt), "mesh_simplify_emit: bad sizes");
    O2345_REQUIRE(workspace && (!verts_out || verts || nv == 0), "mesh_simplify_emit: null pointer");
    SimCarve c;
    (void)sim_carve(workspace, nv, nt, c);
    hipStream_t s = (hipStream_t)stream;
    if (nv > 0 && (verts_out || source || merged))
        hipLaunchKernelGGL(k_sim_emit_verts, dim3(cdiv(nv, 256)), dim3(256), 0, s, verts, (int)nv, c.parent, c.flag, c.vmap, verts_out, source, merged);
    if (nt > 0 && tris_out) with_index_type(index_bytes, tris_out, [&](auto* t) {
        hipLaunchKernelGGL((k_mesh_emit_tris<int, index_type<decltype(t)>>), dim3(cdiv(3 * nt, 256)), dim3(256), 0, s, c.cur, 3 * nt, c.vmap, c.tkeep, c.tmap, t);
    });
    return check_launch("mesh_simplify_emit");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_mesh_simplify() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)k_sim_apply);
}
}  // namespace o2345
