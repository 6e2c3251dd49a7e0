// Connected components of an indexed triangle mesh on the device, and the order-preserving removal of the small ones ("floaters": the detached
// blobs marching cubes finds in a field built from inconsistent views).  Integer / topology work only: exact, deterministic, and equal to the host
// twin (mesh_io.component_labels / filter_components) to the last index.
//
// Definitions
//   component  vertices connected through triangles that share vertex INDICES (marching-cubes vertices are shared per crossing grid edge, so these are
//              the geometric components).  A vertex that no triangle references is a component of its own with 0 faces.
//   label      of a vertex: the smallest vertex index of its component (canonical: independent of thread order).
//   size       of a component: its number of faces.
//   selection  min_faces = n keeps the components with at least n faces; keep_largest keeps only the component with the most faces, ties to the smaller
//              label; both: keep_largest among what min_faces left.  Whenever a selection is active, 0-face components are dropped.  With neither
//              (min_faces <= 0, keep_largest = 0) every vertex and triangle is kept.
//   output     kept vertices and triangles in their original order, vertices renumbered by an exclusive scan of the keep flags, vertex values copied bit
//              for bit, and `kept`: new -> old vertex index, for gathering any per-vertex attribute.  A triangle is kept iff its first vertex is.
//
// Labelling is a lock-free union-find, NOT label propagation (whose sweep count is the mesh diameter: 35,606 sweeps on a 200,000-triangle strip).
// parent[v] <= v always.  A union finds both roots and attaches the LARGER root under the smaller with one atomicCAS on parent[larger]; a failed CAS
// means another thread's CAS succeeded, and the union retries from the new roots: no thread waits for another, and every walk strictly descends, so
// everything terminates.  Path halving stores only values read from an ancestor.  A separate launch then makes parent[v] the root = the label.
// Face counts are integer atomicAdd, the largest component one 64-bit integer atomicMax of (faces << 32 | ~label): order-independent, no float atomics.
#include "mesh_common.h"

namespace o2345 {

// device scalars of one call (workspace head)
struct CcTotals {
    unsigned long long key;                       // max over candidate components of faces << 32 | (0xFFFFFFFF - label); 0: no candidate
    long long nv_kept, nt_kept;                   // written by k_scan_small
    unsigned long long n_components, n_candidates, n_bad;       // n_candidates: components with >= max(min_faces, 1) faces; n_bad: triangles with an index outside [0, nv)
};

struct CcSelect { int active, keep_largest, min_faces; };       // min_faces already >= 1 when active

__global__ __launch_bounds__(256) void k_cc_init(int* __restrict__ parent, int* __restrict__ faces, int nv, CcTotals* __restrict__ tot) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v == 0) *tot = CcTotals{0ull, 0ll, 0ll, 0ull, 0ull, 0ull};
    if (v < nv) { parent[v] = (int)v; faces[v] = 0; }
}

template <typename IDX>
__global__ __launch_bounds__(256) void k_cc_hook(const IDX* __restrict__ tris, long long nt, int nv, int* __restrict__ parent, CcTotals* __restrict__ tot) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int a, b, c;
    if (!mesh_triangle(tris, t, nv, a, b, c)) { atomicAdd(&tot->n_bad, 1ull); return; }
    cc_union(parent, a, b);
    cc_union(parent, b, c);
}

// parent[v] = root(v) = label.  Runs after every hook has finished, so the roots are final.  The walk only READS other vertices' entries and stores
// its own: an entry that already holds its root is never overwritten with a mere ancestor (which halving by a slower thread could do).
__global__ __launch_bounds__(256) void k_cc_flatten(int* __restrict__ parent, int nv, int* __restrict__ labels_out) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    int r = (int)v;
    for (int p = cc_load(parent + r); p != r; p = cc_load(parent + r)) r = p;
    cc_store(parent + v, r);
    if (labels_out) labels_out[v] = r;
}

// faces[label] += 1 per triangle: the lanes of a wave that hold the same label add once (a mesh is mostly ONE component: one atomic per wave, not 64)
template <typename IDX>
__global__ __launch_bounds__(256) void k_cc_faces(const IDX* __restrict__ tris, long long nt, int nv, const int* __restrict__ label, int* __restrict__ faces) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    int a, b, c;
    const bool active = t < nt && mesh_triangle(tris, t, nv, a, b, c);
    const int l = active ? label[a] : -1;
    unsigned long long todo = __ballot(active);
    while (todo) {                                                  // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const int ll = __shfl(l, leader);
        const unsigned long long same = __ballot(active && l == ll);
        if (lane_id() == leader) atomicAdd(faces + ll, __popcll(same));
        todo &= ~same;
    }
}

// one thread per vertex; the roots count the components and bid for "largest"
__global__ __launch_bounds__(256) void k_cc_select(const int* __restrict__ label, const int* __restrict__ faces, int nv, int min_faces, CcTotals* __restrict__ tot) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool root = v < nv && label[v] == (int)v;
    const int f = root ? faces[v] : 0;
    const bool cand = root && f >= (min_faces > 1 ? min_faces : 1);
    wave_count(root, &tot->n_components);
    wave_count(cand, &tot->n_candidates);
    if (cand) atomicMax(&tot->key, ((unsigned long long)(unsigned)f << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)v));
}

__device__ __forceinline__ bool cc_label_kept(const CcSelect& s, int l, const int* __restrict__ faces, unsigned long long key) {
    if (!s.active) return true;
    if (faces[l] < s.min_faces) return false;
    return !s.keep_largest || (unsigned)l == 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
}

// keep flag of item i: a vertex (TRI = false) or a triangle, which follows its first vertex
template <typename IDX, bool TRI>
__device__ __forceinline__ bool cc_item_kept(const CcSelect& s, const IDX* __restrict__ tris, long long i, long long n, int nv, const int* __restrict__ label,
                                             const int* __restrict__ faces, unsigned long long key) {
    if (i >= n) return false;
    if (!TRI) return cc_label_kept(s, label[i], faces, key);
    int a, b, c;
    if (!mesh_triangle(tris, i, nv, a, b, c)) return false;
    return cc_label_kept(s, label[a], faces, key);
}

// kept items per tile of SCAN_TILE -> block_total[blockIdx.x]
template <typename IDX, bool TRI>
__global__ __launch_bounds__(256) void k_cc_keep_count(CcSelect s, const IDX* __restrict__ tris, long long n, int nv, const int* __restrict__ label,
                                                       const int* __restrict__ faces, const CcTotals* __restrict__ tot, int* __restrict__ block_total) {
    __shared__ int lds[5];
    const unsigned long long key = tot->key;
    const long long i0 = (long long)blockIdx.x * SCAN_TILE + threadIdx.x;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) cnt += cc_item_kept<IDX, TRI>(s, tris, i0 + k * 256, n, nv, label, faces, key);
    int total;
    (void)block_scan_excl(cnt, lds, total);
    if (threadIdx.x == 0) block_total[blockIdx.x] = total;
}

// map[i] = new index of item i, or -1 when it is dropped (block_base: the exclusive scan of block_total)
template <typename IDX, bool TRI>
__global__ __launch_bounds__(256) void k_cc_keep_offsets(CcSelect s, const IDX* __restrict__ tris, long long n, int nv, const int* __restrict__ label,
                                                         const int* __restrict__ faces, const CcTotals* __restrict__ tot, const int* __restrict__ block_base,
                                                         int* __restrict__ map) {
    __shared__ int lds[5];
    const unsigned long long key = tot->key;
    const long long i0 = (long long)blockIdx.x * SCAN_TILE + threadIdx.x;
    int run = block_base[blockIdx.x];
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {                            // row k of the tile = 256 consecutive items: coalesced, and in item order
        const long long i = i0 + k * 256;
        const bool kept = cc_item_kept<IDX, TRI>(s, tris, i, n, nv, label, faces, key);
        int total;
        const int at = run + block_scan_excl(kept ? 1 : 0, lds, total);
        if (i < n) map[i] = kept ? at : -1;
        run += total;
    }
}

// one element per thread, coalesced on both sides
__global__ __launch_bounds__(256) void k_cc_emit_verts(const double* __restrict__ verts, long long nv3, const int* __restrict__ vmap, double* __restrict__ verts_out,
                                                       int* __restrict__ kept_out) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= nv3) return;
    const long long v = j / 3;
    const int d = (int)(j - 3 * v);
    const int w = vmap[v];
    if (w < 0) return;
    if (verts_out) verts_out[3 * (long long)w + d] = verts[j];
    if (kept_out && d == 0) kept_out[w] = (int)v;
}

// not k_mesh_emit_tris: the keep flag here is tmap[t] >= 0
template <typename IDX>
__global__ __launch_bounds__(256) void k_cc_emit_tris(const IDX* __restrict__ tris, long long nt3, const int* __restrict__ vmap, const int* __restrict__ tmap,
                                                      IDX* __restrict__ tris_out) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= nt3) return;
    const long long t = j / 3;
    const int d = (int)(j - 3 * t);
    const int w = tmap[t];
    if (w < 0) return;                                              // kept triangles have three in-range vertices of one kept component
    tris_out[3 * (long long)w + d] = (IDX)vmap[tris[j]];
}

struct CcCarve {
    CcTotals* tot;
    int *label, *faces, *vmap, *tmap, *vblock, *tblock;
    unsigned nbv, nbt;
};

// the one walk through the workspace: carves it, or sizes it when ws is null; returns its size
static size_t cc_carve(void* ws, long long nv, long long nt, CcCarve& c) {
    c.nbv = cdiv(nv, SCAN_TILE); c.nbt = cdiv(nt, SCAN_TILE);
    Carver w(ws);
    c.tot = w.take_bytes<CcTotals>(64);
    c.label = w.take<int>(nv);
    c.faces = w.take<int>(nv);
    c.vmap = w.take<int>(nv);
    c.tmap = w.take<int>(nt);
    c.vblock = w.take<int>(c.nbv);
    c.tblock = w.take<int>(c.nbt);
    return w.bytes();
}

static_assert(sizeof(CcTotals) <= 64, "CcTotals must fit the workspace head");

// the emit kernels index 3 * nv coordinates, and min_faces is compared with an int count
static bool cc_sizes_ok(long long nv, long long nt) { return nv >= 0 && nt >= 0 && 3 * nv < (1ll << 31) && nt < (1ll << 31); }

}  // namespace o2345

using namespace o2345;

extern "C" {

size_t o2345_mesh_components_workspace_bytes(long long nv, long long nt) {
    if (nv < 0 || nt < 0) return 0;
    CcCarve c;
    return cc_carve(nullptr, nv, nt, c);
}

// Pass 1 of the two-call protocol: labels, face counts, selection, keep flags and their scans; returns the counts on the HOST (synchronises the
// stream once -- the caller must allocate the outputs).
int o2345_mesh_components_count(const void* tris, int index_bytes, long long nv, long long nt, long long min_faces, int keep_largest, void* workspace,
                                size_t workspace_bytes, int* labels, long long* n_components_host, long long* n_components_kept_host,
                                long long* nv_kept_host, long long* nt_kept_host, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_components_count", index_bytes);
    O2345_REQUIRE(cc_sizes_ok(nv, nt), "mesh_components_count: bad sizes (nv * 3 and nt must stay below 2^31)");
    O2345_REQUIRE(n_components_host && n_components_kept_host && nv_kept_host && nt_kept_host, "mesh_components_count: null pointer");
    O2345_REQUIRE(nt == 0 || tris, "mesh_components_count: null pointer");
    O2345_REQUIRE_WORKSPACE("mesh_components_count", workspace, workspace_bytes, o2345_mesh_components_workspace_bytes(nv, nt));
    CcCarve c;
    (void)cc_carve(workspace, nv, nt, c);
    CcSelect sel;
    sel.active = (min_faces > 0 || keep_largest) ? 1 : 0;
    sel.keep_largest = keep_largest ? 1 : 0;
    sel.min_faces = (int)(min_faces < 1 ? 1 : (min_faces > 0x7FFFFFFFll ? 0x7FFFFFFFll : min_faces));      // nt < 2^31: a larger threshold keeps nothing either way
    hipStream_t s = (hipStream_t)stream;
    const int n = (int)nv;
    const unsigned gv = cdiv(nv > 0 ? nv : 1, 256), gt = cdiv(nt, 256);
    hipLaunchKernelGGL(k_cc_init, dim3(gv), dim3(256), 0, s, c.label, c.faces, n, c.tot);
    if (nt > 0) with_index_type(index_bytes, tris, [&](auto* t) { hipLaunchKernelGGL(k_cc_hook<index_type<decltype(t)>>, dim3(gt), dim3(256), 0, s, t, nt, n, c.label, c.tot); });
    if (nv > 0) hipLaunchKernelGGL(k_cc_flatten, dim3(gv), dim3(256), 0, s, c.label, n, labels);
    if (nt > 0) with_index_type(index_bytes, tris, [&](auto* t) { hipLaunchKernelGGL(k_cc_faces<index_type<decltype(t)>>, dim3(gt), dim3(256), 0, s, t, nt, n, c.label, c.faces); });
    if (nv > 0) {
        hipLaunchKernelGGL(k_cc_select, dim3(gv), dim3(256), 0, s, c.label, c.faces, n, sel.min_faces, c.tot);
        hipLaunchKernelGGL((k_cc_keep_count<int, false>), dim3(c.nbv), dim3(256), 0, s, sel, (const int*)nullptr, nv, n, c.label, c.faces, c.tot, c.vblock);
        hipLaunchKernelGGL(k_scan_small<long long>, dim3(1), dim3(1024), 0, s, c.vblock, (int)c.nbv, &c.tot->nv_kept);
        hipLaunchKernelGGL((k_cc_keep_offsets<int, false>), dim3(c.nbv), dim3(256), 0, s, sel, (const int*)nullptr, nv, n, c.label, c.faces, c.tot, c.vblock, c.vmap);
    }
    if (nt > 0) with_index_type(index_bytes, tris, [&](auto* t) {
        using IDX = index_type<decltype(t)>;
        hipLaunchKernelGGL((k_cc_keep_count<IDX, true>), dim3(c.nbt), dim3(256), 0, s, sel, t, nt, n, c.label, c.faces, c.tot, c.tblock);
        hipLaunchKernelGGL(k_scan_small<long long>, dim3(1), dim3(1024), 0, s, c.tblock, (int)c.nbt, &c.tot->nt_kept);
        hipLaunchKernelGGL((k_cc_keep_offsets<IDX, true>), dim3(c.nbt), dim3(256), 0, s, sel, t, nt, n, c.label, c.faces, c.tot, c.tblock, c.tmap);
    });
    int rc = check_launch("mesh_components_count");
    if (rc) return rc;
    CcTotals h;
    if ((rc = read_totals(h, c.tot, s, "mesh_components_count"))) return rc;
    O2345_REQUIRE(h.n_bad == 0, "mesh_components_count: %llu triangles index outside 0 .. %lld", h.n_bad, nv - 1);
    *n_components_host = (long long)h.n_components;
    *n_components_kept_host = !sel.active ? (long long)h.n_components : sel.keep_largest ? (h.key ? 1 : 0) : (long long)h.n_candidates;
    *nv_kept_host = h.nv_kept;
    *nt_kept_host = h.nt_kept;
    return 0;
}

// Pass 2: emit.  verts fp64 [nv,3] -> verts_out [nv_kept,3]; tris int32 / int64 [nt,3] -> tris_out [nt_kept,3] of the same width, renumbered;
// kept_out int32 [nv_kept].  Any output may be NULL.  Same workspace, untouched since pass 1.
int o2345_mesh_components_emit(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, void* workspace, double* verts_out,
                               void* tris_out, int* kept_out, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_components_emit", index_bytes);
    O2345_REQUIRE(cc_sizes_ok(nv, nt), "mesh_components_emit: bad sizes");
    O2345_REQUIRE(workspace && (!verts_out || verts || nv == 0) && (!tris_out || tris || nt == 0), "mesh_components_emit: null pointer");
    CcCarve c;
    (void)cc_carve(workspace, nv, nt, c);
    hipStream_t s = (hipStream_t)stream;
    if (nv > 0 && (verts_out || kept_out)) hipLaunchKernelGGL(k_cc_emit_verts, dim3(cdiv(3 * nv, 256)), dim3(256), 0, s, verts, 3 * nv, c.vmap, verts_out, kept_out);
    if (nt > 0 && tris_out) with_index_type(index_bytes, tris, [&](auto* t) {
        using IDX = index_type<decltype(t)>;
        hipLaunchKernelGGL(k_cc_emit_tris<IDX>, dim3(cdiv(3 * nt, 256)), dim3(256), 0, s, t, 3 * nt, c.vmap, c.tmap, (IDX*)tris_out);
    });
    return check_launch("mesh_components_emit");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_mesh_components() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)k_cc_flatten);
}
}  // namespace o2345
