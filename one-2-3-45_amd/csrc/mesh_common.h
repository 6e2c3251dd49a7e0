// What the mesh units share (mcubes.hip, mesh_components.hip, mesh_smooth.hip, mesh_decimate.hip, mesh_simplify.hip, mesh_project.hip, mesh_texture.hip,
// mesh_export.hip, mesh_pack.hip): the triangle reader, the wave-level counter, the row sorts, and on the host the workspace carver, the index-width dispatch, the
// three-launch exclusive scan and the read-back of a call's device totals.  Everything is inline or a template: each unit keeps its own code object.
#pragma once
#include "common.h"
#include "block_kernels.h"
#include <type_traits>

namespace o2345 {

constexpr int SCAN_ITEMS = 8;                         // items per thread of the scan kernels
constexpr int SCAN_TILE = IDX_BLOCK * SCAN_ITEMS;     // per block
constexpr int ROW_PAD = 0x7FFFFFFF;                   // sorts behind every vertex index
constexpr int ROW_SHORT = 32;                         // entries of a row that one thread sorts in registers
constexpr int ROW_LONG_GRID = 64;                     // blocks of the long-row kernels (each loops over the list)

// corners of triangle t, narrowed to int -> true iff all three lie in [0, nv)
template <typename IDX>
__device__ __forceinline__ bool mesh_triangle(const IDX* __restrict__ tris, long long t, int nv, int& a, int& b, int& c) {
    const long long ia = (long long)tris[3 * t], ib = (long long)tris[3 * t + 1], ic = (long long)tris[3 * t + 2];
    a = (int)ia; b = (int)ib; c = (int)ic;
    return ia >= 0 && ia < nv && ib >= 0 && ib < nv && ic >= 0 && ic < nv;
}

// *counter += the lanes of this wave with pred: one ballot, and one atomic from lane 0 when any lane has it.  Every lane of the wave must call it.
__device__ __forceinline__ void wave_count(bool pred, unsigned long long* counter) {
    const unsigned long long m = __ballot(pred);
    if (lane_id() == 0 && m) atomicAdd(counter, (unsigned long long)__popcll(m));
}

// the finaliser of splitmix64: keys that differ in high bits only spread too (decimation's tables, simplification's priorities)
__device__ __forceinline__ unsigned long long dec_mix(unsigned long long x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// r = the d <= N entries of row, ascending, then ROW_PAD
template <int N>
__device__ __forceinline__ void row_sorted_regs(const int* __restrict__ row, int d, int (&r)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) r[k] = k < d ? row[k] : ROW_PAD;
    sort_regs<N>(r);
}

// srt[0 .. d) = row[0 .. d) ascending, by one 256-thread block: a stable rank sort (position = entries that are smaller + equal entries in front),
// O(d^2 / 256) comparisons per thread.  srt is complete for the whole block on return, and row is free.  Decimation's member rows are distinct: the
// tie term never fires there, and the result is what "position = members that are smaller" gives, to the bit.
__device__ __forceinline__ void row_rank_sort(const int* row, int* srt, int d) {
    for (int i = threadIdx.x; i < d; i += 256) {
        const int x = row[i];
        int pos = 0;
        for (int j = 0; j < d; ++j) {
            const int y = row[j];
            pos += (y < x || (y == x && j < i)) ? 1 : 0;
        }
        srt[pos] = x;
    }
    __syncthreads();
}

// Bump carver of a workspace.  A unit describes its layout in ONE function that walks a carver; run on a null base the walk is the size
// (o2345_*_workspace_bytes), run on the caller's buffer it yields the pointers: the two cannot drift apart.
struct Carver {
    uintptr_t base;
    size_t off = 0;
    explicit Carver(void* ws) : base((uintptr_t)ws) {}
    // count elements of T, advancing by their size padded to 16 bytes
    template <typename T> T* take(size_t count) { return take_bytes<T>((count * sizeof(T) + 15) / 16 * 16); }
    // exactly `bytes`, unpadded: a head of fixed size, or an array whose size keeps the alignment that the next region needs
    template <typename T> T* take_bytes(size_t bytes) { T* p = (T*)(base + off); off += bytes; return p; }
    void skip(size_t n) { off += n; }
    size_t bytes() const { return off; }
};

// f(typed tris) once, with the triangle array typed by its index width: const int* / const long long*, or without the const for an output array.
// The caller has checked index_bytes (4 or 8).  Inside f, index_type<decltype(typed)> names the element type for the kernel's template argument.
template <typename P> using index_type = std::remove_const_t<std::remove_pointer_t<P>>;
template <typename V, typename F>
void with_index_type(int index_bytes, V* tris, F&& f) {
    static_assert(std::is_void<V>::value, "with_index_type takes the untyped array of the C ABI");
    constexpr bool ro = std::is_const<V>::value;
    if (index_bytes == 4) f((std::conditional_t<ro, const int, int>*)tris);
    else f((std::conditional_t<ro, const long long, long long>*)tris);
}

// exclusive scan of a[0 .. n) -> out (and out2 when not null), the sum -> *total; block_total: cdiv(n, 256 * ITEMS) = blocks ints of scratch
template <int ITEMS>
void exclusive_scan(const int* a, long long n, unsigned blocks, int* block_total, int* out, int* out2, long long* total, hipStream_t s) {
    hipLaunchKernelGGL(k_tile_sum<ITEMS>, dim3(blocks), dim3(256), 0, s, a, n, block_total);
    hipLaunchKernelGGL(k_scan_small<long long>, dim3(1), dim3(1024), 0, s, block_total, (int)blocks, total);
    hipLaunchKernelGGL(k_tile_scan<ITEMS>, dim3(blocks), dim3(256), 0, s, a, n, block_total, out, out2);
}

// the device totals of pass 1 -> totals on the host: one copy, one synchronisation of the stream; a failure is the unit's error string and status
template <typename T>
int read_totals(T& totals, const T* device, hipStream_t s, const char* unit) {
    hipError_t e = hipMemcpyAsync(&totals, device, sizeof(T), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    O2345_REQUIRE(e == hipSuccess, "%s: %s", unit, hipGetErrorString(e));
    return 0;
}

}  // namespace o2345
