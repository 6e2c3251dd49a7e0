// What the mesh units share.  The units: mcubes.hip, mesh_components.hip, mesh_smooth.hip and mesh_simplify.hip (both through mesh_adjacency.h),
// mesh_decimate.hip, mesh_project.hip, mesh_texture.hip, mesh_distance.hip, mesh_audit.hip, mesh_fill.hip, mesh_intersect.hip, mesh_export.hip, mesh_pack.hip, and surface_trace.hip for the wave
// sums and finite().  On the device: the triangle reader, the wave-level counter and reductions, finite(), the order-preserving fp64 <-> uint64 encoding,
// the union-find of the components and the audit, the row
// sorts (registers, the short-row ladder, the block-wide long form) and the kernel that emits kept triangles.  On the host: the workspace carver, the
// entry checks (sizes, index width, workspace), the index-width dispatch, the three-launch exclusive scan and the read-back of a call's device totals.
// The index -> world frame of projection and texture is in mesh_math.h.  Everything is inline, a template or in an anonymous namespace: each unit keeps
// its own code object.
#pragma once
#include "common.h"
#include "block_kernels.h"
#include <float.h>
#include <math.h>
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

// min / max / sum over the 64 lanes of a wave by butterflies (off = 32 .. 1); every lane returns the result, and every lane must call
__device__ __forceinline__ unsigned long long wave_min(unsigned long long x) {
    for (int off = 32; off; off >>= 1) { const unsigned long long y = __shfl_xor(x, off); x = y < x ? y : x; }
    return x;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long x) {
    for (int off = 32; off; off >>= 1) { const unsigned long long y = __shfl_xor(x, off); x = y > x ? y : x; }
    return x;
}
template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
    static_assert(std::is_same<T, int>::value || std::is_same<T, unsigned long long>::value, "integer sums only: a float sum has an order to document");
    for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// neither an infinity nor a NaN.  (At global scope, behind `using namespace o2345`, write o2345::finite: the C library has a function of that name.)
O2345_HD bool finite(double x) { return fabs(x) <= DBL_MAX; }

// fp64 -> uint64 whose unsigned order is the order of the doubles (for integer atomicMin / atomicMax of a bound), and back
__device__ __forceinline__ unsigned long long ordered_bits(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ordered_double(unsigned long long e) {
    return __longlong_as_double((long long)((e >> 63) ? (e & 0x7FFFFFFFFFFFFFFFull) : ~e));
}

// the finaliser of splitmix64: keys that differ in high bits only spread too (decimation's tables, simplification's priorities)
__device__ __forceinline__ unsigned long long dec_mix(unsigned long long x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// Lock-free union-find over int nodes (the vertices of mesh_components.hip, the triangle corners of mesh_audit.hip): parent[x] <= x always, a union
// attaches the LARGER root under the smaller with one atomicCAS, and a later launch reads the roots (see mesh_components.hip for why it terminates).
__device__ __forceinline__ int cc_load(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ void cc_store(int* p, int v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }

// root of x; on the way every visited node is re-pointed to its grandparent (a value read from an ancestor, so parent[.] stays an ancestor whatever
// the interleaving; a non-root never becomes a root again, so these stores never disturb a CAS, which only succeeds on roots)
__device__ __forceinline__ int cc_find(int* parent, int x) {
    int p = cc_load(parent + x);
    while (p != x) {
        const int g = cc_load(parent + p);
        if (g != p) cc_store(parent + x, g);
        x = p; p = g;
    }
    return x;
}

__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        if (atomicCAS(parent + a, a, b) == a) return;          // lost: a is no root any more, go on from the new roots
    }
}

// r = the d <= N entries of row, ascending, then ROW_PAD
template <int N, int STRIDE = 1>
__device__ __forceinline__ void row_sorted_regs(const int* __restrict__ row, int d, int (&r)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) r[k] = k < d ? row[STRIDE * k] : ROW_PAD;
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

// Sorting an unordered CSR row in place.  A kernel with one thread per row lists the rows above ROW_SHORT entries for a second kernel with one block per
// listed row (row_sort_long) and sorts the others itself (row_sort_short); a row of one entry or none is sorted as it is.

// row[0 .. d) ascending, d <= N, by its own thread in registers.  STRIDE: the distance in ints between two entries of the row (one column of an [n, STRIDE]
// array: the pairs of mesh_intersect.hip)
template <int N, int STRIDE = 1>
__device__ __forceinline__ void row_sort_regs_in_place(int* __restrict__ row, int d) {
    int r[N];
    row_sorted_regs<N, STRIDE>(row, d, r);
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (k < d) row[STRIDE * k] = r[k];
}

// row[0 .. d) ascending for 1 < d <= ROW_SHORT: the smallest of three register networks that holds the row
template <int STRIDE = 1>
__device__ __forceinline__ void row_sort_short(int* __restrict__ row, int d) {
    if (d > 16) row_sort_regs_in_place<ROW_SHORT, STRIDE>(row, d);
    else if (d > 4) row_sort_regs_in_place<16, STRIDE>(row, d);
    else row_sort_regs_in_place<4, STRIDE>(row, d);
}

// row[0 .. d) ascending by one 256-thread block: rank sort into tmp, copied back.  On return tmp[0 .. d) is the sorted row, complete for the whole
// block; row[0 .. d) holds the same values once the block's stores have landed (its next barrier, or the kernel's end): a thread that reads other
// threads' entries before that reads tmp.
__device__ __forceinline__ void row_sort_long(int* row, int* tmp, int d) {
    row_rank_sort(row, tmp, d);
    for (int i = threadIdx.x; i < d; i += 256) row[i] = tmp[i];
}

// Kept triangles out: element j = 3 t + k of src goes to out[3 tmap[t] + k], renumbered through map, iff tkeep[t].  src is the input's triangle array
// or a unit's working copy; kept triangles have three in-range corners with a map entry >= 0.  One thread per element, coalesced on both sides.
namespace {
template <typename SRC, typename IDX>
__global__ __launch_bounds__(256) void k_mesh_emit_tris(const SRC* __restrict__ src, long long nt3, const int* __restrict__ map, const int* __restrict__ tkeep,
                                                        const int* __restrict__ tmap, IDX* __restrict__ out) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= nt3) return;
    const long long t = j / 3;
    if (!tkeep[t]) return;
    out[3 * (long long)tmap[t] + (j - 3 * t)] = (IDX)map[src[j]];
}
}  // namespace

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

// Entry checks.  The sizes at which vertex indices fit an int and 3 * nt a 31-bit element count (decimation, distance; the adjacency and the components
// have limits of their own).  The two macros return -1 from the entry with the messages that callers match on; `unit` is a string literal.
inline bool mesh_sizes_ok(long long nv, long long nt) { return nv >= 0 && nt >= 0 && nv < (1ll << 30) && 3 * nt < (1ll << 31); }

#define O2345_REQUIRE_INDEX_BYTES(unit, index_bytes) O2345_REQUIRE((index_bytes) == 4 || (index_bytes) == 8, unit ": index_bytes must be 4 or 8")

// need: the unit's o2345_*_workspace_bytes of the call's sizes, which the entry has checked before
#define O2345_REQUIRE_WORKSPACE(unit, workspace, workspace_bytes, need)                                             \
    do {                                                                                                            \
        O2345_REQUIRE(workspace, unit ": null pointer");                                                            \
        O2345_REQUIRE((workspace_bytes) >= (need), unit ": workspace too small");                                   \
        O2345_REQUIRE(((uintptr_t)(workspace) & 15) == 0, unit ": workspace must be 16-byte aligned");              \
    } while (0)

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
