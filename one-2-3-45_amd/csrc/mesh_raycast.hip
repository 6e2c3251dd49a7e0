// Ray casting against a triangle mesh on the device, and its first user, ambient occlusion: what a segment hits (k_rc_cast: the nearest hit, or whether
// there is any), and how many of S rays about the normal of a point are blocked (k_rc_occlusion).  Through the uniform grid of mesh_distance.hip or
// over every triangle, without one.  t, tri, hits and the counters equal the host twin (mesh_io.ray_cast / mesh_occlusion) to the last bit, whatever
// the grid: every decision is a comparison of fp64 values computed one operation at a time in a defined order (mesh_raycast_math.h), the rest is integer.
//
// Definitions (include/o2345.h has the full text)
//   usable     a triangle takes part iff its three indices lie in [0, nv), its nine coordinates are finite and n . n != 0 (md_normal2: the grid's own rule).
//   hit        mi_segment_hit: P and Q strictly on opposite sides of the triangle's plane, the three determinants about the segment all > 0 or all < 0.  A
//              zero or a NaN anywhere is no hit: a segment through a shared edge or vertex hits neither neighbour (rays leak there).  A segment with a
//              non-finite coordinate hits nothing; a segment of length zero hits nothing by the rule itself.
//   nearest    t = sP / (sP - sQ); the smallest t over the usable triangles that are hit, among equal t the smallest index (rc_nearest); (inf, -1) without.
//   occlusion  point p, direction n (given, or the owner's face normal, or the owner's face normal turned to the given side): frame (T, B, N) of n
//              (rc_frame); ray i from P = p + bias N to Q = P + max_distance d_i, d_i = (x_i T + y_i B) + z_i N of table entry i (rc_occlusion_ray);
//              hits = the number of rays with any hit.
// Walk.  The segment's slabs along its dominant axis a (the largest |Q - P| component), from md_cell_index(P_a) to md_cell_index(Q_a): the one monotone
// index function that registered the triangles, so the slab of every point of the segment lies between the two.  Slab i is entered at t0 and left at t1
// (0 in the first, 1 in the last slab, else where the segment meets the slab's face, clamped to [0, 1]); the other two coordinates of the segment over
// [t0, t1] lie between their values at both ends; that interval, widened on both sides by slack = 2^-30 (head->scale + the largest coordinate of P and
// Q), is mapped through md_cell_index: the rectangle of cells in between, normally 1 to 4, is the slab's visit.  A hit point h is a point of the triangle
// and of the segment: the triangle is registered in the cell of (index(h_x), index(h_y), index(h_z)), whose slab is walked, and h's other two coordinates
// differ from the interval by the rounding of t0, t1 and of the index function, a few 2^-53 of the coordinates times |D_b / D_a| <= 1: a millionth of the
// slack.  So every triangle the segment can hit is visited; visiting one twice changes neither a minimum nor a flag.  A segment outside the grid's box
// is legal: the index function clamps.  |Q - P| overflowing leaves t0, t1 without meaning: every slab then visits its whole rectangle.
// The nearest-hit walk stops before a slab whose t0, minus slack / |D_a|, exceeds the best t; the any-hit walk stops at its first hit.
// Work.  k_rc_cast: one lane per segment.  k_rc_occlusion: one lane per (point, direction), the S directions of a point in consecutive lanes, so a wave
// reads the same few cells; the count is one ballot and, per point-row of the wave, one integer atomicAdd of the popcount by the row's first lane.
// Integers only: no floating-point atomics, no kernel waits for another workgroup, the same bytes on every run.
// Bad input never faults: an index outside [0, nv) is never dereferenced, an owner outside [0, nt) neither; cells, entries and triangle numbers read from
// the grid are clamped to the sizes the caller states, so a grid of another mesh gives wrong results, not a fault.
#include "mesh_grid.h"
#include "mesh_raycast_math.h"

namespace o2345 {

constexpr long long RC_EXHAUSTIVE_MAX = 1ll << 16;    // triangles of the path without a grid
constexpr int RC_MAX_SAMPLES = 1024;                  // directions per point

enum { RC_BAD_POINTS = 0, RC_BAD_FRAMES = 1, RC_RAYS = 2, RC_COUNTERS = 4 };          // mesh_io.OCCLUSION_COUNTS

// v[a] without a dynamically indexed array (which would live in scratch)
__device__ __forceinline__ double rc_pick(const double (&v)[3], int a) { return a == 0 ? v[0] : (a == 1 ? v[1] : v[2]); }

// triangle t against the segment -> the nearest hit so far (ANY: best_t >= 0 is the flag); true: an any-hit walk may stop
template <typename IDX, bool ANY>
__device__ __forceinline__ bool rc_visit(const double (&P)[3], const double (&Q)[3], const double* __restrict__ verts, int nv, const IDX* __restrict__ tris,
                                         long long t, double& best, int& best_t) {
    int a, b, c;
    if (!mesh_triangle(tris, t, nv, a, b, c)) return false;
    double A[3], B[3], C[3], tp;
    if (!md_corners(verts, a, b, c, A, B, C)) return false;
    if (md_normal2(A, B, C) == 0.0) return false;
    if (!rc_segment_triangle(P, Q, A, B, C, tp)) return false;
    if (ANY) { best_t = 0; return true; }
    rc_nearest(tp, (int)t, best, best_t);
    return false;
}

// every triangle in index order: the definition on the device, and the path for tiny meshes
template <typename IDX, bool ANY>
__device__ __forceinline__ void rc_walk_all(const double (&P)[3], const double (&Q)[3], const double* __restrict__ verts, int nv, const IDX* __restrict__ tris,
                                            long long nt, double& best, int& best_t) {
    for (long long t = 0; t < nt; ++t)
        if (rc_visit<IDX, ANY>(P, Q, verts, nv, tris, t, best, best_t)) return;
}

// the slabs of the dominant axis (see "Walk" above)
template <typename IDX, bool ANY>
__device__ __forceinline__ void rc_walk_grid(const double (&P)[3], const double (&Q)[3], const double* __restrict__ verts, int nv, const IDX* __restrict__ tris,
                                             long long nt, const MdGridView& g, double& best, int& best_t) {
    const double D[3] = {Q[0] - P[0], Q[1] - P[1], Q[2] - P[2]};
    const double ad[3] = {fabs(D[0]), fabs(D[1]), fabs(D[2])};
    const int a = (ad[0] >= ad[1] && ad[0] >= ad[2]) ? 0 : (ad[1] >= ad[2] ? 1 : 2);
    const int b = a == 2 ? 0 : a + 1, c = a == 0 ? 2 : a - 1;
    const double Da = rc_pick(D, a), Db = rc_pick(D, b), Dc = rc_pick(D, c);
    if (Da == 0.0) return;                                           // length zero: sP == sQ for every triangle
    const bool wide = !(fabs(Da) <= DBL_MAX);
    const double Pa = rc_pick(P, a), Pb = rc_pick(P, b), Pc = rc_pick(P, c), Qa = rc_pick(Q, a);
    const MdGridHead* __restrict__ head = g.head;
    const double cell = head->cell;
    const int nx = min(max(head->dims[0], 1), MD_AXIS), ny = min(max(head->dims[1], 1), MD_AXIS), nz = min(max(head->dims[2], 1), MD_AXIS);
    const int na = a == 0 ? nx : (a == 1 ? ny : nz), nb = b == 0 ? nx : (b == 1 ? ny : nz), nc = c == 0 ? nx : (c == 1 ? ny : nz);
    const int sa = a == 0 ? 1 : (a == 1 ? nx : nx * ny), sb = b == 0 ? 1 : (b == 1 ? nx : nx * ny), sc = c == 0 ? 1 : (c == 1 ? nx : nx * ny);
    const double oa = head->origin[a], ob = head->origin[b], oc = head->origin[c];
    const double big = fmax(fmax(fabs(P[0]), fabs(P[1])), fmax(fabs(P[2]), fmax(fabs(Q[0]), fmax(fabs(Q[1]), fabs(Q[2])))));      // the largest coordinate of P and Q
    const double slack = (head->scale + big) * MD_SLACK, tslack = slack / fabs(Da);
    const int ia0 = md_cell_index(Pa, oa, cell, na), ia1 = md_cell_index(Qa, oa, cell, na), dir = Da > 0.0 ? 1 : -1;
    const long long last_cell = g.max_cells - 1;
    for (int i = ia0; (ia1 - i) * dir >= 0; i += dir) {
        double t0 = 0.0, t1 = 1.0;
        if (i != ia0) t0 = fmin(fmax(((oa + (double)(dir > 0 ? i : i + 1) * cell) - Pa) / Da, 0.0), 1.0);
        if (i != ia1) t1 = fmin(fmax(((oa + (double)(dir > 0 ? i + 1 : i) * cell) - Pa) / Da, 0.0), 1.0);
        if (!ANY && !wide && t0 - tslack > best) return;
        int jb0 = 0, jb1 = nb - 1, jc0 = 0, jc1 = nc - 1;
        if (!wide) {
            const double b0 = Pb + t0 * Db, b1 = Pb + t1 * Db, c0 = Pc + t0 * Dc, c1 = Pc + t1 * Dc;
            jb0 = md_cell_index(fmin(b0, b1) - slack, ob, cell, nb); jb1 = md_cell_index(fmax(b0, b1) + slack, ob, cell, nb);
            jc0 = md_cell_index(fmin(c0, c1) - slack, oc, cell, nc); jc1 = md_cell_index(fmax(c0, c1) + slack, oc, cell, nc);
        }
        for (int jc = jc0; jc <= jc1; ++jc)
            for (int jb = jb0; jb <= jb1; ++jb) {
                long long ci = (long long)i * sa + (long long)jb * sb + (long long)jc * sc;
                ci = ci > last_cell ? last_cell : ci;                // only in a grid of another mesh
                long long e = g.cell_start[ci], e1 = g.cell_start[ci + 1];
                e = e < 0 ? 0 : e;
                e1 = e1 > g.cap_entries ? g.cap_entries : e1;
                for (; e < e1; ++e) {
                    const long long t = g.entries[e];
                    if (t < 0 || t >= nt) continue;
                    if (rc_visit<IDX, ANY>(P, Q, verts, nv, tris, t, best, best_t)) return;
                }
            }
    }
}

// the segment against the mesh -> (t, tri) of the nearest hit, (inf, -1) without; ANY: tri >= 0 iff anything is hit
template <typename IDX, bool GRID, bool ANY>
__device__ __forceinline__ void rc_trace(const double (&P)[3], const double (&Q)[3], const double* __restrict__ verts, int nv, const IDX* __restrict__ tris,
                                         long long nt, const MdGridView& g, double& best_out, int& best_t_out) {
    double best = INFINITY;                                          // locals, written out once (see md_walk_grid)
    int best_t = -1;
    if (rc_segment_finite(P, Q)) {
        if (GRID) rc_walk_grid<IDX, ANY>(P, Q, verts, nv, tris, nt, g, best, best_t);
        else rc_walk_all<IDX, ANY>(P, Q, verts, nv, tris, nt, best, best_t);
    }
    best_out = best;
    best_t_out = best_t;
}

// one lane per segment.  ANY: tri = 1 / 0 and t is not written
template <typename IDX, bool GRID, bool ANY>
__global__ __launch_bounds__(256) void k_rc_cast(const double* __restrict__ p, const double* __restrict__ q, long long n, const double* __restrict__ verts, int nv,
                                                 const IDX* __restrict__ tris, long long nt, MdGridView g, double* __restrict__ t_out, int* __restrict__ tri_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double P[3] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]}, Q[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
    double best;
    int best_t;
    rc_trace<IDX, GRID, ANY>(P, Q, verts, nv, tris, nt, g, best, best_t);
    if (ANY) tri_out[i] = best_t >= 0 ? 1 : 0;
    else { t_out[i] = best; tri_out[i] = best_t; }
}

// one lane per (point, direction): lane e is direction e % S of point e / S.  hits is zeroed by the entry
template <typename IDX, bool GRID>
__global__ __launch_bounds__(256) void k_rc_occlusion(const double* __restrict__ points, const double* __restrict__ dirs, const int* __restrict__ owners,
                                                      long long n, const double* __restrict__ table, int S, double max_distance, double bias,
                                                      const double* __restrict__ verts, int nv, const IDX* __restrict__ tris, long long nt, MdGridView g,
                                                      int* __restrict__ hits, unsigned long long* __restrict__ counters) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = e < n * S;
    const long long i = live ? e / S : -1;
    const int j = live ? (int)(e - i * S) : 0;
    bool bad_point = false, bad_frame = false, cast = false, hit = false;
    if (live) {
        const double p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        double nrm[3] = {0.0, 0.0, 0.0}, T[3], B[3], N[3];
        bool ok = finite(p[0]) && finite(p[1]) && finite(p[2]);
        bad_point = !ok;
        if (ok && owners) {
            const long long o = owners[i];
            int a, b, c;
            double A[3], Bc[3], C[3];
            ok = o >= 0 && o < nt && mesh_triangle(tris, o, nv, a, b, c) && md_corners(verts, a, b, c, A, Bc, C) && md_normal2(A, Bc, C) != 0.0;
            if (ok) {
                rc_face_normal(A, Bc, C, nrm);
                if (dirs) {
                    const double d[3] = {dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
                    if (md_dot(nrm, d) < 0.0) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
                }
            }
        } else if (ok) {
            nrm[0] = dirs[3 * i]; nrm[1] = dirs[3 * i + 1]; nrm[2] = dirs[3 * i + 2];
        }
        if (ok) ok = rc_frame(nrm, T, B, N);
        bad_frame = !bad_point && !ok;
        if (ok) {
            double P[3], Q[3], best;
            int best_t;
            rc_occlusion_ray(p, T, B, N, table[3 * j], table[3 * j + 1], table[3 * j + 2], max_distance, bias, P, Q);
            rc_trace<IDX, GRID, true>(P, Q, verts, nv, tris, nt, g, best, best_t);
            cast = true;
            hit = best_t >= 0;
        }
    }
    // the rows of this wave: lanes [first, last] hold point i
    const unsigned long long mask = __ballot(hit);
    const int lane = lane_id();
    const long long wave0 = e - lane;
    if (live && (lane == 0 || j == 0) && mask) {
        const long long first = i * S - wave0, last = (i + 1) * S - 1 - wave0;
        const int lo = first < 0 ? 0 : (int)first, hi = last > 63 ? 63 : (int)last;
        const unsigned long long row = (hi == 63 ? ~0ull : ((1ull << (hi + 1)) - 1)) & ~((1ull << lo) - 1);
        const int cnt = __popcll(mask & row);
        if (cnt) atomicAdd(hits + i, cnt);
    }
    wave_count(bad_point && j == 0, counters + RC_BAD_POINTS);
    wave_count(bad_frame && j == 0, counters + RC_BAD_FRAMES);
    wave_count(cast, counters + RC_RAYS);
}

static bool rc_mesh_ok(long long nv, long long nt, const double* verts, const void* tris) { return mesh_sizes_ok(nv, nt) && (nv == 0 || verts) && (nt == 0 || tris); }

}  // namespace o2345

using namespace o2345;

extern "C" {

int o2345_mesh_ray_cast(const double* p, const double* q, long long n, const double* verts, const void* tris, int index_bytes, long long nv, long long nt,
                        const void* grid, size_t grid_bytes, long long max_cells, int any_hit, double* t, int* tri, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_ray_cast", index_bytes);
    O2345_REQUIRE(n >= 0 && n < MD_MAX_SAMPLES && mesh_sizes_ok(nv, nt), "mesh_ray_cast: bad sizes (n < 2^28, nv < 2^30, 3 * nt < 2^31)");
    O2345_REQUIRE((n == 0 || (p && q && tri && (any_hit || t))) && rc_mesh_ok(nv, nt, verts, tris), "mesh_ray_cast: null pointer");
    MdGridView g;
    if (!md_grid_view("mesh_ray_cast", grid, grid_bytes, max_cells, nt, RC_EXHAUSTIVE_MAX, g)) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    with_index_type(index_bytes, tris, [&](auto* tt) {
        using IDX = index_type<decltype(tt)>;
        auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, p, q, n, verts, (int)nv, tt, nt, g, t, tri); };
        if (g.head) { if (any_hit) launch(k_rc_cast<IDX, true, true>); else launch(k_rc_cast<IDX, true, false>); }
        else { if (any_hit) launch(k_rc_cast<IDX, false, true>); else launch(k_rc_cast<IDX, false, false>); }
    });
    return check_launch("mesh_ray_cast");
}

int o2345_mesh_occlusion(const double* points, const double* dirs_or_null, const int* owners_or_null, long long n, const double* table, int n_samples,
                         double max_distance, double bias, const double* verts, const void* tris, int index_bytes, long long nv, long long nt, const void* grid,
                         size_t grid_bytes, long long max_cells, int* hits, long long* counters, void* stream) {
    O2345_REQUIRE_INDEX_BYTES("mesh_occlusion", index_bytes);
    O2345_REQUIRE(n >= 0 && n < MD_MAX_SAMPLES && mesh_sizes_ok(nv, nt), "mesh_occlusion: bad sizes (n < 2^28, nv < 2^30, 3 * nt < 2^31)");
    O2345_REQUIRE(n_samples >= 1 && n_samples <= RC_MAX_SAMPLES, "mesh_occlusion: n_samples must be in 1 .. 1024, got %d", n_samples);
    O2345_REQUIRE(max_distance > 0.0 && max_distance <= DBL_MAX, "mesh_occlusion: max_distance must be a finite float > 0, got %g", max_distance);
    O2345_REQUIRE(bias >= 0.0 && bias <= DBL_MAX, "mesh_occlusion: bias must be a finite float >= 0, got %g", bias);
    O2345_REQUIRE(counters && table && (n == 0 || (points && hits)) && rc_mesh_ok(nv, nt, verts, tris), "mesh_occlusion: null pointer");
    O2345_REQUIRE(n == 0 || dirs_or_null || owners_or_null, "mesh_occlusion: a point needs a direction or an owner triangle");
    O2345_REQUIRE(((uintptr_t)counters & 7) == 0, "mesh_occlusion: counters must be 8-byte aligned");
    MdGridView g;
    if (!md_grid_view("mesh_occlusion", grid, grid_bytes, max_cells, nt, RC_EXHAUSTIVE_MAX, g)) return -1;
    hipStream_t s = (hipStream_t)stream;
    O2345_HIP(hipMemsetAsync(counters, 0, RC_COUNTERS * sizeof(long long), s));
    if (n == 0) return 0;
    O2345_HIP(hipMemsetAsync(hits, 0, (size_t)n * sizeof(int), s));
    with_index_type(index_bytes, tris, [&](auto* tt) {
        using IDX = index_type<decltype(tt)>;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(cdiv(n * n_samples, 256)), dim3(256), 0, s, points, dirs_or_null, owners_or_null, n, table, n_samples, max_distance, bias,
                               verts, (int)nv, tt, nt, g, hits, (unsigned long long*)counters);
        };
        if (g.head) launch(k_rc_occlusion<IDX, true>); else launch(k_rc_occlusion<IDX, false>);
    });
    return check_launch("mesh_occlusion");
}

}  // extern "C"

// o2345_preload (csrc/api.cpp): querying one kernel makes the HIP runtime load this translation unit's code object on the current device
namespace o2345 {
int preload_mesh_raycast() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)k_rc_cast<int, false, true>);
}
}  // namespace o2345
