// Asset export (replaces utils/utils.py:31-47, convert_mesh_format: trimesh.load_mesh(mesh.ply) -> two rotations + an x flip + reversed faces ->
// mesh.obj / mesh.glb): the buffers of a binary glTF and the text of a vertex-coloured Wavefront OBJ, produced on the device from the marching-cubes
// output, so that export is one D2H copy per buffer and one file write -- the design of mesh_pack.hip extended to the two formats viewers load.
//   frame:   the reference's three matrices compose to the exact swap (x, y, z) -> (x, z, y) (a reflection: z-up -> glTF's y-up) and it reverses every
//            face (a, b, c) -> (c, b, a); positions are therefore the PLY's float32 positions (mesh_math.h, shared with k_pack_vertices) with columns
//            1 and 2 exchanged, bit for bit.
//   GLB:     float32 positions + their per-axis min / max (required on the POSITION accessor), uint8 rgba, optional float32 unit normals, uint32 indices.
//   OBJ:     fixed-width records (record i of a kind starts at i * len: no scan), built per block in LDS and copied out in 16-byte pieces.
#include "common.h"
#include "mesh_math.h"
#include <string.h>
#include <thread>
#include <vector>

namespace o2345 {

// min / max of six per-thread values over a 256-thread block -> red[0..5] valid in threads 0..5 after the call (lds: 4 x 6 floats)
__device__ __forceinline__ void block_minmax(float mn[3], float mx[3], float* lds, float out[6]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            mn[d] = fminf(mn[d], __shfl_xor(mn[d], off));
            mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], off));
        }
    }
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { lds[w * 6 + d] = mn[d]; lds[w * 6 + 3 + d] = mx[d]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        float r = lds[k];
        for (int i = 1; i < 4; ++i) r = k < 3 ? fminf(r, lds[i * 6 + k]) : fmaxf(r, lds[i * 6 + k]);
        out[k] = r;
    }
}

// One vertex per thread: position (swapped), rgba, unit normal (swapped); per-block min / max of the float32 positions -> partials[block][6]
__global__ __launch_bounds__(256) void k_asset_vertices(const double* __restrict__ vidx, long long n, MeshXform x, const float* __restrict__ rgb,
                                                        const float* __restrict__ grad, float* __restrict__ pos, uint8_t* __restrict__ rgba,
                                                        float* __restrict__ nrm, float* __restrict__ partials) {
    __shared__ float red[24];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < n) {
        float f[3];
        mesh_vertex_f32(vidx, i, x, f);
        const float p[3] = {f[0], f[2], f[1]};
#pragma unroll
        for (int d = 0; d < 3; ++d) { pos[3 * i + d] = p[d]; mn[d] = p[d]; mx[d] = p[d]; }
        if (rgb) {
            const uchar4 c = make_uchar4(mesh_colour_u8(rgb[3 * i]), mesh_colour_u8(rgb[3 * i + 1]), mesh_colour_u8(rgb[3 * i + 2]), 255);
            *reinterpret_cast<uchar4*>(rgba + 4 * i) = c;
        }
        if (grad) {
            // normalize(g) -> 3x3 of trans_mat -> renormalise, in fp64; scale_mat is a positive uniform scale and leaves a direction alone
            double g[3] = {(double)grad[3 * i], (double)grad[3 * i + 1], (double)grad[3 * i + 2]};
            double l = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
            bool ok = l > 0.0 && l < (double)INFINITY;
            if (ok) {
                g[0] /= l; g[1] /= l; g[2] /= l;
                if (x.has_trans) {
                    double w[3];
#pragma unroll
                    for (int r = 0; r < 3; ++r) w[r] = (x.T[4 * r] * g[0] + x.T[4 * r + 1] * g[1]) + x.T[4 * r + 2] * g[2];
                    l = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
                    ok = l > 0.0 && l < (double)INFINITY;
                    g[0] = w[0] / l; g[1] = w[1] / l; g[2] = w[2] / l;
                }
            }
            nrm[3 * i] = ok ? (float)g[0] : 0.f;
            nrm[3 * i + 1] = ok ? (float)g[2] : 1.f;
            nrm[3 * i + 2] = ok ? (float)g[1] : 0.f;
        }
    }
    float out[6];
    block_minmax(mn, mx, red, out);
    if (threadIdx.x < 6) partials[(long long)blockIdx.x * 6 + threadIdx.x] = out[threadIdx.x];
}

// second stage: ONE block folds the per-block partials -> bounds[0..2] = min, bounds[3..5] = max (min / max are exact: any order gives the same bits)
__global__ __launch_bounds__(256) void k_asset_bounds_finish(const float* __restrict__ partials, long long nblocks, float* __restrict__ bounds) {
    __shared__ float red[24];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long b = threadIdx.x; b < nblocks; b += 256) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { mn[d] = fminf(mn[d], partials[b * 6 + d]); mx[d] = fmaxf(mx[d], partials[b * 6 + 3 + d]); }
    }
    float out[6];
    block_minmax(mn, mx, red, out);
    if (threadIdx.x < 6) bounds[threadIdx.x] = out[threadIdx.x];
}

// out[i] = (c, b, a) of triangle i as uint32: one element per thread, coalesced on both sides
template <typename IDX>
__global__ __launch_bounds__(256) void k_asset_indices(const IDX* __restrict__ tris, long long m3, uint32_t* __restrict__ out) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= m3) return;
    const long long t = j / 3;
    const int d = (int)(j - 3 * t);
    out[j] = (uint32_t)tris[3 * t + (2 - d)];
}

// 256 records of one kind per block.  Each thread formats its record into LDS at the byte phase the block's output has in global memory
// (so a 16-byte piece of LDS is a 16-byte aligned piece of the file), then the block copies head bytes / uint4 body / tail bytes.
constexpr int OBJ_KIND_V = 0, OBJ_KIND_VN = 1, OBJ_KIND_F = 2, OBJ_TABLE_BYTES = 256 * 11;
__global__ __launch_bounds__(256) void k_obj_records(int kind, ObjLayout L, const float* __restrict__ pos, const uint8_t* __restrict__ rgba,
                                                     const float* __restrict__ nrm, const uint32_t* __restrict__ idx,
                                                     const uint8_t* __restrict__ table, long long count, uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];         // colour table (2,816 = 176 x 16 bytes) | 16 + 256 * len: all LDS is dynamic,
    uint8_t* tab = lds;                                                   // so the staging area starts 16-byte aligned
    uint8_t* stage = lds + OBJ_TABLE_BYTES;
    const int len = kind == OBJ_KIND_V ? L.v_len : kind == OBJ_KIND_VN ? L.vn_len : L.f_len;
    const long long r0 = (long long)blockIdx.x * 256;
    const int nrec = (int)(count - r0 < 256 ? count - r0 : 256);
    uint8_t* g = out + r0 * len;
    const int phase = (int)((uintptr_t)g & 15);
    const int tid = threadIdx.x;
    if (kind == OBJ_KIND_V && L.colours) {
        for (int k = 0; k < 11; ++k) tab[tid * 11 + k] = table[tid * 11 + k];
        __syncthreads();
    }
    if (tid < nrec) {
        const long long i = r0 + tid;
        uint8_t* dst = stage + phase + tid * len;
        if (kind == OBJ_KIND_V) {
            const float p[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
            uint8_t c[4] = {0, 0, 0, 0};
            if (L.colours) __builtin_memcpy(c, rgba + 4 * i, 4);
            obj_vertex_record(dst, L, p, c, tab);
        } else if (kind == OBJ_KIND_VN) {
            const float p[3] = {nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
            obj_normal_record(dst, p);
        } else {
            const uint32_t t[3] = {idx[3 * i], idx[3 * i + 1], idx[3 * i + 2]};
            obj_face_record(dst, L, t);
        }
    }
    __syncthreads();
    const int bytes = nrec * len;
    int head = phase ? 16 - phase : 0;
    if (head > bytes) head = bytes;
    const int nvec = (bytes - head) >> 4;
    const int tail = bytes - head - (nvec << 4);
    if (tid < head) g[tid] = stage[phase + tid];
    const uint4* sv = reinterpret_cast<const uint4*>(stage + phase + head);           // phase + head is 0 or 16 when nvec > 0
    uint4* gv = reinterpret_cast<uint4*>(g + head);
    for (int v = tid; v < nvec; v += 256) gv[v] = sv[v];
    const int t0 = head + (nvec << 4);
    if (tid < tail) g[t0 + tid] = stage[phase + t0 + tid];
}

static void obj_colour_table(uint8_t* table /*[256 * 11]*/) {
    char b[16];
    for (int c = 0; c < 256; ++c) { snprintf(b, sizeof b, " %.8f", (double)c / 255.0); memcpy(table + 11 * c, b, 11); }
}

}  // namespace o2345

using namespace o2345;

extern "C" {

size_t o2345_mesh_bounds_workspace_bytes(long long n) { return n <= 0 ? 0 : (size_t)cdiv(n, 256) * 6 * sizeof(float); }

int o2345_mesh_asset_vertices(const double* verts_idx, long long n, int grid_R, const float* bound_min, const float* bound_max, const float* scale_mat,
                              const float* trans_mat, const float* rgb, const float* grad, float* positions, uint8_t* rgba, float* normals,
                              float* bounds, void* workspace, size_t workspace_bytes, void* stream) {
    O2345_REQUIRE(bound_min && bound_max && grid_R >= 2, "mesh_asset_vertices: bad bounds / resolution");
    if (n <= 0) return 0;
    O2345_REQUIRE(verts_idx && positions && bounds && workspace, "mesh_asset_vertices: null pointer");
    O2345_REQUIRE((!rgb || rgba) && (!grad || normals), "mesh_asset_vertices: rgb needs rgba, grad needs normals");
    O2345_REQUIRE(workspace_bytes >= o2345_mesh_bounds_workspace_bytes(n), "mesh_asset_vertices: workspace of %zu bytes, need %zu", workspace_bytes,
                  o2345_mesh_bounds_workspace_bytes(n));
    O2345_REQUIRE(((uintptr_t)workspace & 3) == 0 && (!rgba || ((uintptr_t)rgba & 3) == 0), "mesh_asset_vertices: workspace / rgba must be 4-byte aligned");
    const MeshXform x = mesh_xform(grid_R, bound_min, bound_max, scale_mat, trans_mat);
    const unsigned nb = cdiv(n, 256);
    hipLaunchKernelGGL(k_asset_vertices, dim3(nb), dim3(256), 0, (hipStream_t)stream, verts_idx, n, x, rgb, grad, positions, rgba, normals, (float*)workspace);
    hipLaunchKernelGGL(k_asset_bounds_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, (long long)nb, bounds);
    return check_launch("mesh_asset_vertices");
}

int o2345_mesh_asset_indices(const void* tris, int index_bytes, long long m, uint32_t* indices, void* stream) {
    O2345_REQUIRE(index_bytes == 4 || index_bytes == 8, "mesh_asset_indices: index_bytes must be 4 or 8");
    if (m <= 0) return 0;
    O2345_REQUIRE(tris && indices, "mesh_asset_indices: null pointer");
    if (index_bytes == 8) hipLaunchKernelGGL(k_asset_indices<long long>, dim3(cdiv(3 * m, 256)), dim3(256), 0, (hipStream_t)stream, (const long long*)tris, 3 * m, indices);
    else hipLaunchKernelGGL(k_asset_indices<int32_t>, dim3(cdiv(3 * m, 256)), dim3(256), 0, (hipStream_t)stream, (const int32_t*)tris, 3 * m, indices);
    return check_launch("mesh_asset_indices");
}

size_t o2345_obj_text_bytes(long long n, long long m, int K, int colors, int normals) {
    if (n < 0 || m < 0 || K < 1 || K > 9) return 0;
    const ObjLayout L = obj_layout(n, K, colors, normals);
    return (size_t)n * L.v_len + (normals ? (size_t)n * L.vn_len : 0) + (size_t)m * L.f_len;
}

int o2345_obj_text(const float* positions, const uint8_t* rgba, const float* normals, long long n, const uint32_t* indices, long long m, int K,
                   const uint8_t* color_table, uint8_t* text, void* stream) {
    O2345_REQUIRE(K >= 1 && K <= 9, "obj_text: K = %d integer digits (1 .. 9)", K);
    O2345_REQUIRE(n >= 0 && m >= 0 && n < 4294967295ll, "obj_text: bad sizes");
    O2345_REQUIRE((n == 0 || positions) && (m == 0 || indices) && (n + m == 0 || text) && (!rgba || color_table), "obj_text: null pointer");
    O2345_REQUIRE(!rgba || ((uintptr_t)rgba & 3) == 0, "obj_text: rgba must be 4-byte aligned");
    const ObjLayout L = obj_layout(n, K, rgba != nullptr, normals != nullptr);
    uint8_t* o = text;
    auto launch = [&](int kind, long long count, int len) {
        if (count > 0) hipLaunchKernelGGL(k_obj_records, dim3(cdiv(count, 256)), dim3(256), (size_t)(OBJ_TABLE_BYTES + 16 + 256 * len), (hipStream_t)stream, kind, L, positions, rgba, normals, indices,
                                          color_table, count, o);
        o += count * len;
    };
    launch(OBJ_KIND_V, n, L.v_len);
    if (normals) launch(OBJ_KIND_VN, n, L.vn_len);
    launch(OBJ_KIND_F, m, L.f_len);
    return check_launch("obj_text");
}

int o2345_obj_text_host(const float* positions, const uint8_t* rgba, const float* normals, long long n, const uint32_t* indices, long long m, int K,
                        uint8_t* text) {
    O2345_REQUIRE(K >= 1 && K <= 9, "obj_text_host: K = %d integer digits (1 .. 9)", K);
    O2345_REQUIRE(n >= 0 && m >= 0 && n < 4294967295ll, "obj_text_host: bad sizes");
    O2345_REQUIRE((n == 0 || positions) && (m == 0 || indices) && (n + m == 0 || text), "obj_text_host: null pointer");
    const ObjLayout L = obj_layout(n, K, rgba != nullptr, normals != nullptr);
    uint8_t table[256 * 11];
    obj_colour_table(table);
    uint8_t* vn0 = text + n * L.v_len;
    uint8_t* f0 = vn0 + (normals ? n * L.vn_len : 0);
    const uint8_t* tab = table;
    auto part = [=](long long v0, long long v1, long long t0, long long t1) {
        for (long long i = v0; i < v1; ++i) {
            obj_vertex_record(text + i * L.v_len, L, positions + 3 * i, rgba ? rgba + 4 * i : nullptr, tab);
            if (normals) obj_normal_record(vn0 + i * L.vn_len, normals + 3 * i);
        }
        for (long long i = t0; i < t1; ++i) obj_face_record(f0 + i * L.f_len, L, indices + 3 * i);
    };
    const int nt = (n + m) > (1 << 16) ? 4 : 1;
    if (nt == 1) { part(0, n, 0, m); return 0; }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back([=] { part(n * t / nt, n * (t + 1) / nt, m * t / nt, m * (t + 1) / nt); });
    for (auto& t : th) t.join();
    return 0;
}

}  // extern "C"

namespace o2345 {
int preload_mesh_export() {
    hipFuncAttributes at;
    return (int)hipFuncGetAttributes(&at, (const void*)(k_obj_records));
}
}  // namespace o2345
