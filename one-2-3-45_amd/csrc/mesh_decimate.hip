// Decimation of an indexed triangle mesh by vertex clustering (Rossignac - Borrel) on the device: the vertices of one lattice cell of edge `cell` become
// one vertex at their mean, triangles that collapse are dropped, and of several triangles over the same three cells the first stays.  Equal to the host
// twin (mesh_io.decimate_mesh) to the last bit: integer and topology work, plus one sequential fp64 sum per cluster in a defined order.
//
// Definitions
//   cell of v  q = floor(p / cell) per axis in fp64 (IEEE division); two vertices are in one cluster iff their three q are equal.  Per axis max q - min q
//              must be below 2^21: r = q - min q is then an exact integer of 21 bits and (r_x, r_y, r_z) packs into a 63-bit key.  The shift only
//              packs; the partition is that of q, so negative coordinates are legal.
//   rep        the representative of a cluster: its smallest member index.
//   triangles  (a, b, c) maps to (rep a, rep b, rep c).  Degenerate = two mapped corners equal: dropped.  Of the others, those with the same SET of three
//              representatives are duplicates whatever their orientation or rotation: the first in face order is kept.  Kept triangles keep their
//              face order, corner order and orientation.
//   vertices   a cluster is kept iff a kept triangle references it; kept clusters are numbered by an exclusive scan of "is a kept representative" over
//              the old vertex order; cluster[v] = that number, or -1.  Position, per coordinate: acc = 0; acc = acc + p[u] over the members u in
//              ascending index order, one sequential sum; acc / count.
//   Not promised: manifoldness.  Where a thin part collapses, clustering leaves edges with more than two triangles, or open ones.
//
// Why thread order does not matter.  Clusters: an open-addressing table of 64-bit keys (atomicCAS, linear probing from a mixed hash); WHICH slot a key
// lands in depends on timing, its value does not: an integer atomicMin of the vertex index.  Duplicates: a second table whose slots hold a triangle
// index; a thread claims an empty slot with atomicCAS, or compares its sorted triple with that of the triangle the slot holds (all holders of one slot
// have the same set, so the set of a slot never changes) and does atomicMin(slot, t); a triangle is kept iff its slot ends up holding its own index =
// the first in face order.  The cell bounds are integer atomicMin / atomicMax of an order-preserving encoding of q.  Member lists are filled through an
// atomic cursor in any order and then sorted, rows of up to ROW_SHORT members in registers, longer ones by one block each (rank sort).  The sum itself is
// one thread per cluster adding in row order.  No float atomics; every probe loop is bounded by its table's capacity (running out is an error status).
// Inside the two inserting kernels every access to a table is an atomic; plain loads of the tables happen in later launches only.
#include "mesh_common.h"

namespace o2345 {

constexpr unsigned long long DEC_EMPTY = ~0ull;       // key of an empty cluster slot (a packed key has 63 bits)
constexpr double DEC_EXTENT = 2097152.0;              // 2^21 cells per axis

// device scalars of one call (workspace head)
struct DecTotals {
    unsigned long long qmin[3], qmax[3];              // ordered_bits of the per-axis bounds of q
    long long nv_out, nt_out, n_members;              // written by k_scan_small (n_members: the length of the member table, unused otherwise)
    unsigned long long n_nonfinite, n_bad, n_overflow;          // vertices with a non-finite coordinate; triangles with an index outside [0, nv); probes that ran out
    unsigned long long n_clusters, n_degenerate, n_duplicate;
    int bad_extent, n_long;
};

// q of one coordinate; + 0.0 turns floor's -0.0 into +0.0, so that equal q have equal encodings
__device__ __forceinline__ double dec_cell(double p, double cell) { return __dadd_rn(floor(__ddiv_rn(p, cell)), 0.0); }

__device__ __forceinline__ void dec_sort3(int& x, int& y, int& z) {
    regs_cmpswap(x, y); regs_cmpswap(y, z); regs_cmpswap(x, y);
}

// one thread per slot / vertex / triangle of whichever array is longest
__global__ __launch_bounds__(256) void k_dec_init(unsigned long long* __restrict__ keys, int* __restrict__ vals, long long vcap, int* __restrict__ tslots,
                                                  long long tcap, int* __restrict__ flag, int* __restrict__ cnt, int nv, DecTotals* __restrict__ tot) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        DecTotals z = {};
        for (int d = 0; d < 3; ++d) z.qmin[d] = ~0ull;
        *tot = z;
    }
    if (i < vcap) { keys[i] = DEC_EMPTY; vals[i] = ROW_PAD; }          // above every vertex index: the atomicMin of k_dec_insert replaces it
    if (i < tcap) tslots[i] = -1;
    if (i < nv) { flag[i] = 0; cnt[i] = 0; }
}

// per-axis bounds of q, and the count of vertices with a non-finite coordinate
__global__ __launch_bounds__(256) void k_dec_bounds(const double* __restrict__ verts, int nv, double cell, DecTotals* __restrict__ tot) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool active = v < nv;
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
    bool nonfinite = false;
    if (active) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double p = verts[3 * v + d];
            nonfinite |= !finite(p);
            lo[d] = hi[d] = ordered_bits(dec_cell(p, cell));
        }
    }
    const unsigned long long mn = __ballot(nonfinite);
#pragma unroll
    for (int d = 0; d < 3; ++d) { lo[d] = wave_min(lo[d]); hi[d] = wave_max(hi[d]); }
    if (lane_id() == 0 && active) {                                 // lane 0 is the first vertex of its wave: active iff the wave has any vertex
        if (mn) atomicAdd(&tot->n_nonfinite, (unsigned long long)__popcll(mn));
#pragma unroll
        for (int d = 0; d < 3; ++d) { atomicMin(&tot->qmin[d], lo[d]); atomicMax(&tot->qmax[d], hi[d]); }
    }
}

// every vertex inserts its key; vals[slot] = min over the vertices of that key.  A key that cannot be formed (non-finite input, extent too large: an
// error status on the host either way) is clamped into range, so that nothing downstream sees an index it cannot use.
__global__ __launch_bounds__(256) void k_dec_insert(const double* __restrict__ verts, int nv, double cell, unsigned long long* __restrict__ keys,
                                                    int* __restrict__ vals, unsigned mask, unsigned* __restrict__ slot, DecTotals* __restrict__ tot) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    unsigned long long key = 0;
    bool wide = false;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double q0 = ordered_double(tot->qmin[d]);
        wide |= !(__dsub_rn(ordered_double(tot->qmax[d]), q0) < DEC_EXTENT);
        double r = __dsub_rn(dec_cell(verts[3 * v + d], cell), q0);
        r = (r >= 0.0 && r < DEC_EXTENT) ? r : 0.0;
        key = (key << 21) | (unsigned long long)(long long)r;
    }
    if (v == 0 && wide) tot->bad_extent = 1;
    unsigned s = (unsigned)dec_mix(key) & mask;
    for (unsigned i = 0;; ++i) {
        const unsigned long long prev = atomicCAS(keys + s, DEC_EMPTY, key);
        if (prev == DEC_EMPTY || prev == key) {
            atomicMin(vals + s, (int)v);
            slot[v] = s;
            return;
        }
        if (i == mask) break;                                       // every slot seen
        s = (s + 1) & mask;
    }
    atomicAdd(&tot->n_overflow, 1ull);
    slot[v] = 0;
}

// rep[v] from the finished table (plain loads: a later launch); the representatives count the clusters
__global__ __launch_bounds__(256) void k_dec_rep(const int* __restrict__ vals, const unsigned* __restrict__ slot, int nv, int* __restrict__ rep,
                                                 DecTotals* __restrict__ tot) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    int r = -1;
    if (v < nv) {
        r = vals[slot[v]];
        if (r < 0 || r > v) r = (int)v;                             // only after a probe ran out (an error status): keep every index usable
        rep[v] = r;
    }
    wave_count(v < nv && r == (int)v, &tot->n_clusters);
}

// tslot[t] = the slot of triangle t's set of representatives in the second table, or -1 for a degenerate (or unusable) triangle
template <typename IDX>
__global__ __launch_bounds__(256) void k_dec_tris(const IDX* __restrict__ tris, long long nt, int nv, const int* __restrict__ rep, int* __restrict__ tslots,
                                                  unsigned mask, int* __restrict__ tslot, DecTotals* __restrict__ tot) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false, degenerate = false, lost = false;
    if (t < nt) {
        int a, b, c, state = -1;
        if (!mesh_triangle(tris, t, nv, a, b, c)) bad = true;
        else {
            int x = rep[a], y = rep[b], z = rep[c];
            if (x == y || y == z || x == z) degenerate = true;
            else {
                dec_sort3(x, y, z);
                unsigned s = (unsigned)dec_mix(dec_mix(((unsigned long long)(unsigned)x << 32) | (unsigned)y) + (unsigned)z) & mask;
                lost = true;
                for (unsigned i = 0;; ++i) {
                    int cur = __atomic_load_n(tslots + s, __ATOMIC_RELAXED);
                    if (cur < 0) cur = atomicCAS(tslots + s, -1, (int)t);
                    if (cur < 0) { state = (int)s; lost = false; break; }          // claimed an empty slot
                    int a2, b2, c2;                                     // the slot holds triangle cur: in range and not degenerate, or it would not be there
                    (void)mesh_triangle(tris, cur, nv, a2, b2, c2);
                    int x2 = rep[a2], y2 = rep[b2], z2 = rep[c2];
                    dec_sort3(x2, y2, z2);
                    if (x2 == x && y2 == y && z2 == z) {
                        atomicMin(tslots + s, (int)t);
                        state = (int)s; lost = false;
                        break;
                    }
                    if (i == mask) break;                               // every slot seen
                    s = (s + 1) & mask;
                }
            }
        }
        tslot[t] = state;
    }
    wave_count(bad, &tot->n_bad);
    wave_count(degenerate, &tot->n_degenerate);
    wave_count(lost, &tot->n_overflow);
}

// tkeep[t] = 1 iff the slot of t holds t; the kept triangles flag the representatives they reference (every writer stores the same 1)
template <typename IDX>
__global__ __launch_bounds__(256) void k_dec_keep(const IDX* __restrict__ tris, long long nt, const int* __restrict__ rep, const int* __restrict__ tslots,
                                                  const int* __restrict__ tslot, int* __restrict__ tkeep, int* __restrict__ flag, DecTotals* __restrict__ tot) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    bool duplicate = false;
    if (t < nt) {
        const int s = tslot[t];
        const bool kept = s >= 0 && tslots[s] == (int)t;
        duplicate = s >= 0 && !kept;
        tkeep[t] = kept ? 1 : 0;
        if (kept) {                                                 // tslot >= 0: the three indices are in range
            flag[rep[tris[3 * t]]] = 1; flag[rep[tris[3 * t + 1]]] = 1; flag[rep[tris[3 * t + 2]]] = 1;
        }
    }
    wave_count(duplicate, &tot->n_duplicate);
}

// cluster_of[v] = the new index of v's cluster or -1; cnt[new index] = its members
__global__ __launch_bounds__(256) void k_dec_assign(int nv, const int* __restrict__ rep, const int* __restrict__ flag, const int* __restrict__ vmap,
                                                    int* __restrict__ cluster_of, int* __restrict__ cnt) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const int r = rep[v];
    const int c = flag[r] ? vmap[r] : -1;
    cluster_of[v] = c;
    if (c >= 0) atomicAdd(cnt + c, 1);
}

// cursor[c] starts at the row's first slot and ends behind its last; the order inside a row is arbitrary until k_dec_rows
__global__ __launch_bounds__(256) void k_dec_fill(int nv, const int* __restrict__ cluster_of, int* __restrict__ cursor, int* __restrict__ members) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const int c = cluster_of[v];
    if (c >= 0) members[atomicAdd(cursor + c, 1)] = (int)v;
}

// one thread per row (rows behind the last kept cluster are empty): short rows are sorted here, long ones are listed
__global__ __launch_bounds__(256) void k_dec_rows(int nv, const int* __restrict__ off, const int* __restrict__ cnt, int* __restrict__ members,
                                                  int* __restrict__ long_list, DecTotals* __restrict__ tot) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= nv) return;
    const int d = cnt[c];
    if (d > ROW_SHORT) long_list[atomicAdd(&tot->n_long, 1)] = (int)c;
    else if (d > 1) row_sort_short(members + off[c], d);
}

// one block per listed row (row_sort_long): the slow path of a mesh with thousands of vertices in one cell
__global__ __launch_bounds__(256) void k_dec_long_rows(const int* __restrict__ off, const int* __restrict__ cnt, int* __restrict__ members, int* __restrict__ tmp,
                                                       const int* __restrict__ long_list, const DecTotals* __restrict__ tot) {
    const int n_long = tot->n_long;
    for (int r = blockIdx.x; r < n_long; r += gridDim.x) {
        const int c = long_list[r];
        const int base = off[c], d = cnt[c];
        row_sort_long(members + base, tmp + base, d);
    }
}

// thread i: cluster[i] for vertex i, and the position of new vertex i: the sequential sum over its row.  -ffp-contract=off (build.py) and the explicit
// _rn forms keep it the twin's sum
__global__ __launch_bounds__(256) void k_dec_emit_verts(const double* __restrict__ verts, int nv, const int* __restrict__ cluster_of, const int* __restrict__ off,
                                                        const int* __restrict__ cnt, const int* __restrict__ members, const DecTotals* __restrict__ tot,
                                                        double* __restrict__ verts_out, int* __restrict__ cluster_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    if (cluster_out) cluster_out[i] = cluster_of[i];
    if (!verts_out || i >= tot->nv_out) return;
    const int lo = off[i], d = cnt[i];
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int k = 0; k < d; ++k) {
        const long long u = members[lo + k];
        ax = __dadd_rn(ax, verts[3 * u]);
        ay = __dadd_rn(ay, verts[3 * u + 1]);
        az = __dadd_rn(az, verts[3 * u + 2]);
    }
    const double n = (double)d;
    verts_out[3 * i] = __ddiv_rn(ax, n); verts_out[3 * i + 1] = __ddiv_rn(ay, n); verts_out[3 * i + 2] = __ddiv_rn(az, n);
}

struct DecCarve {
    DecTotals* tot;
    unsigned long long* keys;
    int *vals, *tslots, *rep, *flag, *vmap, *cluster_of, *cnt, *off, *cursor, *long_list, *members, *tmp, *tslot, *tkeep, *tmap, *vblock, *tblock;
    unsigned* slot;
    long long vcap, tcap;
    unsigned nbv, nbt;
};

static long long dec_capacity(long long n) {                        // the power of two >= 2 n (and >= 2)
    long long c = 2;
    while (c < 2 * n) c <<= 1;
    return c;
}

static_assert(sizeof(DecTotals) <= 128, "DecTotals must fit the workspace head");

// the one walk through the workspace: carves it, or sizes it when ws is null; returns its size
static size_t dec_carve(void* ws, long long nv, long long nt, DecCarve& c) {
    c.vcap = dec_capacity(nv); c.tcap = dec_capacity(nt);
    c.nbv = cdiv(nv, SCAN_TILE); c.nbt = cdiv(nt, SCAN_TILE);
    Carver w(ws);
    c.tot = w.take_bytes<DecTotals>(128);
    c.keys = w.take_bytes<unsigned long long>((size_t)c.vcap * sizeof(unsigned long long));      // the tables: powers of two, unpadded (8 bytes at the
    c.vals = w.take_bytes<int>((size_t)c.vcap * sizeof(int));                                    // smallest, which keeps every int array behind aligned)
    c.tslots = w.take_bytes<int>((size_t)c.tcap * sizeof(int));
    c.slot = w.take<unsigned>(nv);
    for (int** a : {&c.rep, &c.flag, &c.vmap, &c.cluster_of, &c.cnt, &c.off, &c.cursor, &c.long_list, &c.members, &c.tmp}) *a = w.take<int>(nv);
    for (int** a : {&c.tslot, &c.tkeep, &c.tmap}) *a = w.take<int>(nt);
    c.vblock = w.take<int>(c.nbv);
    c.tblock = w.take<int>(c.nbt);
    return w.bytes();
}

}  // namespace o2345

using namespace o2345;

extern "C" {

size_t o2345_mesh_decimate_workspace_bytes(long long nv, long long nt) {
    if (!mesh_sizes_ok(nv, nt)) return 0;
    DecCarve c;
    return dec_carve(nullptr, nv, nt, c);
}

// Pass 1 of the two-call protocol: clusters, kept triangles, renumbering and the sorted member rows, all inside the workspace; returns the counts on
// the HOST (synchronises the stream once -- the caller must allocate the outputs).
int o2345_mesh_decimate_count(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, double cell, void* workspace,
                              size_t workspace_bytes, long long* n_clusters_host, long long* nv_out_host, long long* nt_out_host,
                              long long* n_degenerate_host, long long* n_duplicate_host, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_decimate_count", index_bytes);
    O2345_REQUIRE(cell > 0.0 && o2345::finite(cell), "mesh_decimate_count: cell must be finite and > 0, got %g", cell);
    O2345_REQUIRE(mesh_sizes_ok(nv, nt), "mesh_decimate_count: bad sizes (nv must stay below 2^30 and 3 * nt below 2^31)");
    O2345_REQUIRE(n_clusters_host && nv_out_host && nt_out_host && n_degenerate_host && n_duplicate_host, "mesh_decimate_count: null pointer");
    O2345_REQUIRE((nv == 0 || verts) && (nt == 0 || tris), "mesh_decimate_count: null pointer");
    O2345_REQUIRE_WORKSPACE("mesh_decimate_count", workspace, workspace_bytes, o2345_mesh_decimate_workspace_bytes(nv, nt));
    DecCarve c;
    (void)dec_carve(workspace, nv, nt, c);
    hipStream_t s = (hipStream_t)stream;
    const int n = (int)nv;
    const unsigned gv = cdiv(nv, 256), gt = cdiv(nt, 256);
    const unsigned vmask = (unsigned)(c.vcap - 1), tmask = (unsigned)(c.tcap - 1);
    const long long longest = c.vcap > c.tcap ? c.vcap : c.tcap;     // >= nv as well
    hipLaunchKernelGGL(k_dec_init, dim3(cdiv(longest, 256)), dim3(256), 0, s, c.keys, c.vals, c.vcap, c.tslots, c.tcap, c.flag, c.cnt, n, c.tot);
    if (nv > 0) {
        hipLaunchKernelGGL(k_dec_bounds, dim3(gv), dim3(256), 0, s, verts, n, cell, c.tot);
        hipLaunchKernelGGL(k_dec_insert, dim3(gv), dim3(256), 0, s, verts, n, cell, c.keys, c.vals, vmask, c.slot, c.tot);
        hipLaunchKernelGGL(k_dec_rep, dim3(gv), dim3(256), 0, s, c.vals, c.slot, n, c.rep, c.tot);
    }
    if (nt > 0) {
        with_index_type(index_bytes, tris, [&](auto* t) {
            using IDX = index_type<decltype(t)>;
            hipLaunchKernelGGL(k_dec_tris<IDX>, dim3(gt), dim3(256), 0, s, t, nt, n, c.rep, c.tslots, tmask, c.tslot, c.tot);
            hipLaunchKernelGGL(k_dec_keep<IDX>, dim3(gt), dim3(256), 0, s, t, nt, c.rep, c.tslots, c.tslot, c.tkeep, c.flag, c.tot);
        });
        exclusive_scan<SCAN_ITEMS>(c.tkeep, nt, c.nbt, c.tblock, c.tmap, nullptr, &c.tot->nt_out, s);
    }
    if (nv > 0) {
        exclusive_scan<SCAN_ITEMS>(c.flag, nv, c.nbv, c.vblock, c.vmap, nullptr, &c.tot->nv_out, s);
        hipLaunchKernelGGL(k_dec_assign, dim3(gv), dim3(256), 0, s, n, c.rep, c.flag, c.vmap, c.cluster_of, c.cnt);
        exclusive_scan<SCAN_ITEMS>(c.cnt, nv, c.nbv, c.vblock, c.off, c.cursor, &c.tot->n_members, s);
        hipLaunchKernelGGL(k_dec_fill, dim3(gv), dim3(256), 0, s, n, c.cluster_of, c.cursor, c.members);
        hipLaunchKernelGGL(k_dec_rows, dim3(gv), dim3(256), 0, s, n, c.off, c.cnt, c.members, c.long_list, c.tot);
        hipLaunchKernelGGL(k_dec_long_rows, dim3(ROW_LONG_GRID), dim3(256), 0, s, c.off, c.cnt, c.members, c.tmp, c.long_list, c.tot);
    }
    int rc = check_launch("mesh_decimate_count");
    if (rc) return rc;
    DecTotals h;
    if ((rc = read_totals(h, c.tot, s, "mesh_decimate_count"))) return rc;
    O2345_REQUIRE(h.n_nonfinite == 0, "mesh_decimate_count: %llu vertices have a non-finite coordinate", h.n_nonfinite);
    O2345_REQUIRE(h.n_bad == 0, "mesh_decimate_count: %llu triangles index outside 0 .. %lld", h.n_bad, nv - 1);
    O2345_REQUIRE(h.bad_extent == 0, "mesh_decimate_count: the mesh extends over 2^21 cells or more of size %g along an axis", cell);
    O2345_REQUIRE(h.n_overflow == 0, "mesh_decimate_count: %llu probes found no slot (internal error)", h.n_overflow);
    *n_clusters_host = (long long)h.n_clusters;
    *nv_out_host = h.nv_out;
    *nt_out_host = h.nt_out;
    *n_degenerate_host = (long long)h.n_degenerate;
    *n_duplicate_host = (long long)h.n_duplicate;
    return 0;
}

// Pass 2: verts_out fp64 [nv_out,3], tris_out [nt_out,3] of the input's width, cluster int32 [nv], from the workspace of pass 1 (same nv and nt,
// untouched in between).  Any output may be NULL.
int o2345_mesh_decimate_emit(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, void* workspace, double* verts_out,
                             void* tris_out, int* cluster, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_decimate_emit", index_bytes);
    O2345_REQUIRE(mesh_sizes_ok(nv, nt), "mesh_decimate_emit: bad sizes");
    O2345_REQUIRE(workspace && (!verts_out || verts || nv == 0) && (!tris_out || tris || nt == 0), "mesh_decimate_emit: null pointer");
    DecCarve c;
    (void)dec_carve(workspace, nv, nt, c);
    hipStream_t s = (hipStream_t)stream;
    if (nv > 0 && (verts_out || cluster))
        hipLaunchKernelGGL(k_dec_emit_verts, dim3(cdiv(nv, 256)), dim3(256), 0, s, verts, (int)nv, c.cluster_of, c.off, c.cnt, c.members, c.tot, verts_out, cluster);
    if (nt > 0 && tris_out) with_index_type(index_bytes, tris, [&](auto* t) {
        using IDX = index_type<decltype(t)>;
        hipLaunchKernelGGL((k_mesh_emit_tris<IDX, IDX>), dim3(cdiv(3 * nt, 256)), dim3(256), 0, s, t, 3 * nt, c.cluster_of, c.tkeep, c.tmap, (IDX*)tris_out);
    });
    return check_launch("mesh_decimate_emit");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_mesh_decimate() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)k_dec_rep);
}
}  // namespace o2345
