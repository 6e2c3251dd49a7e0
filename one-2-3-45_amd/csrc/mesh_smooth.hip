// The CSR entries of the vertex adjacency (the table itself: mesh_adjacency.h, shared with mesh_simplify.hip), and Taubin's lambda|mu smoothing of the
// vertex positions over it.  Equal to the host twin (mesh_io.vertex_adjacency / smooth_vertices) to the last bit: the table is integer work, the smoothing
// step is a sequential fp64 sum in a defined order (ascending neighbour index) followed by one division, one subtraction, one multiplication and one
// addition, never fused.
//
// Definitions (rows and boundary: mesh_adjacency.h)
//   step(f)    Jacobi: for every v from the OLD positions, per coordinate acc = 0; acc = acc + p[u] for u ascending; m = acc / deg; d = m - p[v];
//              p'[v] = p[v] + f * d.  deg = 0, or boundary[v] with pinning on: p'[v] = p[v] bit for bit.
//   smooth     `iterations` times: step(lam), then step(mu) unless mu == 0.
#include "mesh_adjacency.h"

namespace o2345 {

// CSR out: one thread per vertex copies its row unless the row is on the long list (raw count above ROW_SHORT); the ROW_LONG_GRID blocks behind the
// vertex blocks copy the listed rows, one block per row (an empty list costs them one load)
__global__ __launch_bounds__(256) void k_adj_emit(int nv, unsigned vertex_blocks, const int* __restrict__ rawoff, const int* __restrict__ cursor,
                                                  const int* __restrict__ deg, const int* __restrict__ off, const int* __restrict__ raw,
                                                  const unsigned char* __restrict__ bnd, const int* __restrict__ long_list, const AdjTotals* __restrict__ tot,
                                                  int* __restrict__ offsets, int* __restrict__ neighbours, unsigned char* __restrict__ boundary) {
    if (blockIdx.x >= vertex_blocks) {
        const int n_long = tot->n_long;
        for (int r = blockIdx.x - vertex_blocks; r < n_long; r += gridDim.x - vertex_blocks) {
            const int v = long_list[r];
            const int d = deg[v], o = off[v], base = rawoff[v];
            for (int k = threadIdx.x; k < d; k += 256) neighbours[o + k] = raw[base + k];
        }
        return;
    }
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v == nv) offsets[nv] = (int)tot->n_entries;
    if (v >= nv) return;
    const int o = off[v], base = rawoff[v];
    offsets[v] = o;
    boundary[v] = bnd[v];
    if (cursor[v] - base > ROW_SHORT) return;
    const int d = deg[v];
    for (int k = 0; k < d; ++k) neighbours[o + k] = raw[base + k];
}

// one Jacobi step with factor f, one thread per vertex; -ffp-contract=off (build.py) and the explicit _rn forms keep multiply and add apart
__global__ __launch_bounds__(256) void k_smooth_step(const double* __restrict__ pin, double* __restrict__ pout, int nv, const int* __restrict__ offsets,
                                                     const int* __restrict__ neighbours, const unsigned char* __restrict__ boundary, double f) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const int lo = offsets[v], hi = offsets[v + 1];
    const double px = pin[3 * v], py = pin[3 * v + 1], pz = pin[3 * v + 2];
    double ox = px, oy = py, oz = pz;
    if (hi > lo && !(boundary && boundary[v])) {
        double ax = 0.0, ay = 0.0, az = 0.0;
        for (int k = lo; k < hi; ++k) {
            const long long u = neighbours[k];
            ax = __dadd_rn(ax, pin[3 * u]);
            ay = __dadd_rn(ay, pin[3 * u + 1]);
            az = __dadd_rn(az, pin[3 * u + 2]);
        }
        const double deg = (double)(hi - lo);
        ox = __dadd_rn(px, __dmul_rn(f, __dsub_rn(__ddiv_rn(ax, deg), px)));
        oy = __dadd_rn(py, __dmul_rn(f, __dsub_rn(__ddiv_rn(ay, deg), py)));
        oz = __dadd_rn(pz, __dmul_rn(f, __dsub_rn(__ddiv_rn(az, deg), pz)));
    }
    pout[3 * v] = ox; pout[3 * v + 1] = oy; pout[3 * v + 2] = oz;
}

}  // namespace o2345

using namespace o2345;

extern "C" {

size_t o2345_mesh_adjacency_workspace_bytes(long long nv, long long nt) {
    if (!adj_sizes_ok(nv, nt)) return 0;
    AdjCarve c;
    return adj_carve(nullptr, nv, nt, c);
}

// Pass 1 of the two-call protocol: the whole build into the workspace; returns the number of CSR entries on the HOST (synchronises the stream once --
// the caller must allocate `neighbours`).
int o2345_mesh_adjacency_count(const void* tris, int index_bytes, long long nv, long long nt, void* workspace, size_t workspace_bytes, long long* n_entries_host,
                               void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_adjacency_count", index_bytes);
    O2345_REQUIRE(adj_sizes_ok(nv, nt), "mesh_adjacency_count: bad sizes (nv must stay below 2^30 and 6 * nt below 2^31)");
    O2345_REQUIRE(n_entries_host && (nt == 0 || tris), "mesh_adjacency_count: null pointer");
    O2345_REQUIRE_WORKSPACE("mesh_adjacency_count", workspace, workspace_bytes, o2345_mesh_adjacency_workspace_bytes(nv, nt));
    AdjCarve c;
    (void)adj_carve(workspace, nv, nt, c);
    hipStream_t s = (hipStream_t)stream;
    with_index_type(index_bytes, tris, [&](auto* t) { adj_build(t, nv, nt, c, s); });
    int rc = check_launch("mesh_adjacency_count");
    if (rc) return rc;
    AdjTotals h;
    if ((rc = read_totals(h, c.tot, s, "mesh_adjacency_count"))) return rc;
    O2345_REQUIRE(h.n_bad == 0, "mesh_adjacency_count: %llu triangles index outside 0 .. %lld", h.n_bad, nv - 1);
    *n_entries_host = h.n_entries;
    return 0;
}

// Pass 2: offsets int32 [nv + 1], neighbours int32 [n_entries], boundary uint8 [nv], from the workspace of pass 1 (same nv, untouched in between).
// neighbours may be NULL when the table is empty.
int o2345_mesh_adjacency_emit(void* workspace, long long nv, int* offsets, int* neighbours, unsigned char* boundary, void* stream) {
    O2345_REQUIRE(nv >= 0 && nv < (1ll << 30), "mesh_adjacency_emit: bad sizes");
    O2345_REQUIRE(workspace && offsets && (nv == 0 || boundary), "mesh_adjacency_emit: null pointer");
    AdjCarve c;
    (void)adj_carve(workspace, nv, 0, c);                          // nt = 0: see adj_carve
    const unsigned vertex_blocks = cdiv(nv + 1, 256);
    hipLaunchKernelGGL(k_adj_emit, dim3(vertex_blocks + ROW_LONG_GRID), dim3(256), 0, (hipStream_t)stream, (int)nv, vertex_blocks, c.rawoff, c.cursor, c.cap, c.off, c.raw,
                       c.bnd, c.long_list, c.tot, offsets, neighbours, boundary);
    return check_launch("mesh_adjacency_emit");
}

// `iterations` times step(lam) [, step(mu) unless mu == 0], ping-pong between verts_tmp and verts_out so that the last step writes verts_out;
// verts_in is only read.  iterations == 0 copies.  verts_tmp may be NULL when there is a single step or none.
int o2345_mesh_smooth(const double* verts_in, long long nv, const int* offsets, const int* neighbours, const unsigned char* boundary_or_null, int iterations,
                      double lam, double mu, double* verts_tmp, double* verts_out, void* stream) {
    O2345_REQUIRE(nv >= 0 && nv < (1ll << 30), "mesh_smooth: bad sizes (nv must stay below 2^30)");
    O2345_REQUIRE(iterations >= 0, "mesh_smooth: iterations must be >= 0, got %d", iterations);
    O2345_REQUIRE(lam > 0.0 && lam <= 1.0 && mu <= 0.0 && o2345::finite(mu), "mesh_smooth: need 0 < lam <= 1 and finite mu <= 0, got %g, %g", lam, mu);
    const long long steps = (long long)iterations * (mu != 0.0 ? 2 : 1);
    O2345_REQUIRE(nv == 0 || (verts_in && verts_out && offsets && (steps < 2 || verts_tmp)), "mesh_smooth: null pointer");
    if (nv == 0) return 0;
    O2345_REQUIRE(verts_out != verts_in && verts_tmp != verts_in && verts_tmp != verts_out, "mesh_smooth: verts_in, verts_tmp and verts_out must differ");
    hipStream_t s = (hipStream_t)stream;
    if (steps == 0) {
        O2345_HIP(hipMemcpyAsync(verts_out, verts_in, (size_t)nv * 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    const double* src = verts_in;
    for (long long i = 0; i < steps; ++i) {
        double* dst = ((steps - 1 - i) & 1) ? verts_tmp : verts_out;
        const double f = (mu != 0.0 && (i & 1)) ? mu : lam;
        hipLaunchKernelGGL(k_smooth_step, dim3(cdiv(nv, 256)), dim3(256), 0, s, src, dst, (int)nv, offsets, neighbours, boundary_or_null, f);
        src = dst;
    }
    return check_launch("mesh_smooth");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_mesh_smooth() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)k_smooth_step);
}
}  // namespace o2345
