// Asset export (replaces utils/utils.py:31-47, convert_mesh_format: trimesh.load_mesh(mesh.ply) -> two rotations + an x flip + reversed faces ->
// mesh.obj / mesh.glb): the buffers of a binary glTF and the text of a vertex-coloured Wavefront OBJ, produced on the device from the marching-cubes
// output, so that export is one D2H copy per buffer and one file write -- the design of mesh_pack.hip extended to the two formats viewers load.
//   frame:   the reference's three matrices compose to the exact swap (x, y, z) -> (x, z, y) (a reflection: z-up -> glTF's y-up) and it reverses every
//            face (a, b, c) -> (c, b, a); positions are therefore the PLY's float32 positions (mesh_math.h, shared with k_pack_vertices) with columns
//            1 and 2 exchanged, bit for bit.
//   GLB:     float32 positions + their per-axis min / max (required on the POSITION accessor), uint8 rgba, optional float32 unit normals, uint32 indices.
//   OBJ:     fixed-width records (record i of a kind starts at i * len: no scan), built per block in LDS and copied out in 16-byte pieces.
#include "mesh_common.h"
#include "mesh_math.h"
#include <string.h>
#include <thread>
#include <vector>

namespace o2345 {

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
            float nn[3];
            mesh_normal_f32(grad, i, x, nn);                 // mesh_math.h: shared with the textured corners (mesh_texture.hip)
            nrm[3 * i] = nn[0]; nrm[3 * i + 1] = nn[1]; nrm[3 * i + 2] = nn[2];
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
// Kinds VT ("vt u v" of the textured file) and FT (its "f a/a b/b c/c" over unwelded corners, which needs no index buffer) came with mesh_texture.hip.
constexpr int OBJ_KIND_V = 0, OBJ_KIND_VN = 1, OBJ_KIND_F = 2, OBJ_KIND_VT = 3, OBJ_KIND_FT = 4, OBJ_TABLE_BYTES = 256 * 11;
__global__ __launch_bounds__(256) void k_obj_records(int kind, ObjLayout L, const float* __restrict__ pos, const uint8_t* __restrict__ rgba,
                                                     const float* __restrict__ nrm, const uint32_t* __restrict__ idx, const float* __restrict__ uv,
                                                     const uint8_t* __restrict__ table, long long count, uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];         // colour table (2,816 = 176 x 16 bytes) | 16 + 256 * len: all LDS is dynamic,
    uint8_t* tab = lds;                                                   // so the staging area starts 16-byte aligned
    uint8_t* stage = lds + OBJ_TABLE_BYTES;
    const int len = kind == OBJ_KIND_V ? L.v_len : kind == OBJ_KIND_VN ? L.vn_len : kind == OBJ_KIND_F ? L.f_len : kind == OBJ_KIND_VT ? L.vt_len : L.ft_len;
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
        } else if (kind == OBJ_KIND_F) {
            const uint32_t t[3] = {idx[3 * i], idx[3 * i + 1], idx[3 * i + 2]};
            obj_face_record(dst, L, t);
        } else if (kind == OBJ_KIND_VT) {
            const float t[2] = {uv[2 * i], uv[2 * i + 1]};
            obj_texcoord_record(dst, t);
        } else {
            obj_corner_face_record(dst, L, (unsigned)i);
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

void mesh_bounds_finish(const float* partials, long long nblocks, float* bounds, hipStream_t stream) {
    hipLaunchKernelGGL(k_asset_bounds_finish, dim3(1), dim3(256), 0, stream, partials, nblocks, bounds);
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
    mesh_bounds_finish((const float*)workspace, (long long)nb, bounds, (hipStream_t)stream);
    return check_launch("mesh_asset_vertices");
}

int o2345_mesh_asset_indices(const void* tris, int index_bytes, long long m, uint32_t* indices, void* stream) {
    O2345_REQUIRE(index_bytes == 4 || index_bytes == 8, "mesh_asset_indices: index_bytes must be 4 or 8");
    if (m <= 0) return 0;
    O2345_REQUIRE(tris && indices, "mesh_asset_indices: null pointer");
    with_index_type(index_bytes, tris, [&](auto* t) { hipLaunchKernelGGL(k_asset_indices<index_type<decltype(t)>>, dim3(cdiv(3 * m, 256)), dim3(256), 0, (hipStream_t)stream, t, 3 * m, indices); });
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
                                          (const float*)nullptr, color_table, count, o);
        o += count * len;
    };
    launch(OBJ_KIND_V, n, L.v_len);
    if (normals) launch(OBJ_KIND_VN, n, L.vn_len);
    launch(OBJ_KIND_F, m, L.f_len);
    return check_launch("obj_text");
}

size_t o2345_obj_texture_text_bytes(long long n, int K, int normals) {
    if (n < 0 || n % 3 || K < 1 || K > 9) return 0;
    const ObjLayout L = obj_layout(n, K, 0, normals);
    return (size_t)n * L.v_len + (size_t)n * L.vt_len + (normals ? (size_t)n * L.vn_len : 0) + (size_t)(n / 3) * L.ft_len;
}

int o2345_obj_texture_text(const float* positions, const float* uv, const float* normals, long long n, int K, uint8_t* text, void* stream) {
    O2345_REQUIRE(K >= 1 && K <= 9, "obj_texture_text: K = %d integer digits (1 .. 9)", K);
    O2345_REQUIRE(n >= 0 && n % 3 == 0 && n < 4294967295ll, "obj_texture_text: bad size (n = 3 x triangles, below 2^32)");
    O2345_REQUIRE(n == 0 || (positions && uv && text), "obj_texture_text: null pointer");
    const ObjLayout L = obj_layout(n, K, 0, normals != nullptr);
    uint8_t* o = text;
    auto launch = [&](int kind, long long count, int len) {
        if (count > 0) hipLaunchKernelGGL(k_obj_records, dim3(cdiv(count, 256)), dim3(256), (size_t)(OBJ_TABLE_BYTES + 16 + 256 * len), (hipStream_t)stream, kind, L, positions,
                                          (const uint8_t*)nullptr, normals, (const uint32_t*)nullptr, uv, (const uint8_t*)nullptr, count, o);
        o += count * len;
    };
    launch(OBJ_KIND_V, n, L.v_len);
    launch(OBJ_KIND_VT, n, L.vt_len);
    if (normals) launch(OBJ_KIND_VN, n, L.vn_len);
    launch(OBJ_KIND_FT, n / 3, L.ft_len);
    return check_launch("obj_texture_text");
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
