// Shared helpers for the o2345 HIP library (gfx950 only).
#pragma once
#include "../../include/o2345.h"      // every translation unit sees the public prototypes: an entry point that drifts from the header does not compile
#include <atomic>
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#define O2345_HD __host__ __device__ __forceinline__

namespace o2345 {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return -2;
    }
    return 0;
}

#define O2345_REQUIRE(cond, ...)            \
    do {                                    \
        if (!(cond)) {                      \
            o2345::set_error(__VA_ARGS__);  \
            return -1;                      \
        }                                   \
    } while (0)

// runtime calls on the way to a launch (memset, attribute queries): failure -> error string + status, like O2345_REQUIRE
#define O2345_HIP(call)                                                               \
    do {                                                                              \
        const hipError_t e_ = (call);                                                 \
        if (e_ != hipSuccess) {                                                       \
            o2345::set_error("%s: %s", #call, hipGetErrorString(e_));                 \
            return -2;                                                                \
        }                                                                             \
    } while (0)

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// Compute units of the CURRENT device (the one the caller's stream belongs to), cached per device ordinal: persistent kernels
// size their grids from it, and one process may drive several GPUs.
inline int cu_count() {
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cached[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev] = n;
    }
    return cached[dev];
}

// wave64 helpers --------------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return __lane_id(); }

// exclusive prefix of a 1-bit predicate inside the wave + wave total (ballot + popcount; no LDS)
__device__ __forceinline__ int wave_prefix(bool pred, int& total) {
    unsigned long long m = __ballot(pred);
    total = __popcll(m);
    return __popcll(m & ((1ull << lane_id()) - 1ull));
}

// exclusive prefix of a 1-bit predicate over a 256/512/1024-thread block; returns block total via ref
template <int NWAVES>
__device__ __forceinline__ int block_prefix(bool pred, int* lds_wave_tot /*[NWAVES+1]*/, int& block_total) {
    int wtot;
    int p = wave_prefix(pred, wtot);
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) lds_wave_tot[w] = wtot;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NWAVES; ++i) {
        int t = lds_wave_tot[i];
        if (i < w) base += t;
        tot += t;
    }
    block_total = tot;
    __syncthreads();
    return base + p;
}


// Debug / A-B knobs of the library, read from the environment ONCE (first use; function-local static: thread-safe, and no getenv on a launch path --
// getenv is not safe against a concurrent setenv, and the library is used from one host thread per stream / device):
//   O2345_LIST_SORT=0     render call: keep the occupied-point list in emission order (no grouping by view-visibility signature)
//   O2345_COLOR_SCHED=n   scheduling and skipping bits of the colour kernel (color_net.h), default 10
//   O2345_SPARSE_BRICK=0  finest sparse convolution in the gather form instead of the LDS-tiled brick form
//   O2345_FLAT_SCHED=1    persistent network kernels: flat block-interleaved tile schedule (odd grid) instead of one eighth of the list per XCD
//   O2345_COLOR_KERNEL=tiles  (only in a -DO2345_TILES_KERNEL test build) the (point, view)-column colour kernel instead of k_color_pts
//   O2345_RAY_STREAM_MIN=n  render call: ray batches of at least n rays run the streaming sampler kernels (one lane per ray, lists read from global
//                         memory at full occupancy), smaller ones the sixteen-lanes-per-ray kernels (default 4096; 0 = always streaming, a huge value = never)
//   O2345_TILE_QUEUE=0    render call: the persistent network kernels run their static tile schedule alone (no tile queue for the tail; A/B switch)
struct Knobs {
    bool list_sort, sparse_brick, flat_sched, color_tiles;
    int color_sched;
    long long ray_stream_min;
    bool tile_queue;
};
inline const Knobs& knobs() {
    static const Knobs k = [] {
        auto is = [](const char* name, char c) { const char* e = getenv(name); return e && e[0] == c; };
        const char* cs = getenv("O2345_COLOR_SCHED");
        const char* rs = getenv("O2345_RAY_STREAM_MIN");
        return Knobs{!is("O2345_LIST_SORT", '0'), !is("O2345_SPARSE_BRICK", '0'), is("O2345_FLAT_SCHED", '1'), is("O2345_COLOR_KERNEL", 't'), cs ? atoi(cs) : 10,
                     rs ? atoll(rs) : 4096, !is("O2345_TILE_QUEUE", '0')};
    }();
    return k;
}

// hipFuncAttributeMaxDynamicSharedMemorySize of a kernel, raised at most once per (call site, device, size): call sites keep one `MaxLds` object
// (function-local static).  Replaces a hipFuncSetAttribute on every launch.
struct MaxLds {
    std::atomic<int> cur[64];
    MaxLds() { for (auto& c : cur) c.store(0, std::memory_order_relaxed); }
    hipError_t ensure(const void* func, size_t bytes) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if ((int)bytes <= cur[dev].load(std::memory_order_acquire)) return hipSuccess;
        const hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e == hipSuccess) cur[dev].store((int)bytes, std::memory_order_release);
        return e;
    }
};
#define O2345_ENSURE_LDS(kernel, bytes)                                                   \
    do {                                                                                  \
        static o2345::MaxLds max_lds_;                                                    \
        O2345_HIP(max_lds_.ensure((const void*)(kernel), (size_t)(bytes)));               \
    } while (0)

// host side: grid of a persistent network kernel.  O2345_FLAT_SCHED=1 (debug / A-B knob) makes the grid odd, which selects the
// flat block-interleaved schedule in tile_schedule() below.
inline unsigned persistent_grid(long long want, int n_cu) {
    unsigned g = (unsigned)(want < n_cu ? want : n_cu);
    if (knobs().flat_sched && g > 8 && (g & 7) == 0) --g;
    return g;
}

// host side: grid of a persistent network kernel whose workgroups of `threads` threads take `units_per_wave` units (points, rays) per wave and tile;
// with a device-side count (n_dev) the size is unknown here and every compute unit gets a workgroup
inline unsigned network_grid(long long n, const void* n_dev, int threads, int units_per_wave) {
    const int n_cu = cu_count();
    const long long per_block = (long long)(threads / 64) * units_per_wave;
    return persistent_grid(n_dev ? n_cu : (n + per_block - 1) / per_block, n_cu);
}

// Tile schedule of the persistent network kernels.  Workgroups are dispatched round-robin over the 8 XCDs (block b runs on XCD
// b % 8) and every XCD has its own 4 MB L2: handing consecutive tiles to consecutive blocks makes each XCD stream the whole
// working set (source-view maps, latent volume) through its L2.  Instead every XCD gets one contiguous eighth of the tile list
// (neighbouring rays / samples share map pixels and voxels), interleaved over its own blocks and waves.
struct TileSched { long long first, end, stride; };
O2345_HD TileSched tile_schedule_flat_at(long long ntiles, int block, int grid, int wave, int nwave) {      // block-interleaved over the whole list
    return {(long long)block * nwave + wave, ntiles, (long long)grid * nwave};
}
O2345_HD TileSched tile_schedule_at(long long ntiles, int block, int grid, int wave, int nwave) {
    if ((grid & 7) == 0) {
        const int xcd = block & 7, slot = block >> 3, per_xcd = grid >> 3;
        const long long chunk = (ntiles + 7) / 8, lo = xcd * chunk, hi = lo + chunk;
        return {lo + (long long)slot * nwave + wave, hi < ntiles ? hi : ntiles, (long long)per_xcd * nwave};
    }
    return tile_schedule_flat_at(ntiles, block, grid, wave, nwave);
}

// Tile queue: the static schedule above ends a kernel when its slowest wave ends.  With a queue (eight int32 heads in caller memory, zero at launch) only
// tiles [0, n_static) are dealt statically -- the same number to every wave -- and the tail [n_static, n_tiles) is claimed, C consecutive tiles per claim, by
// whichever wave has finished its share.  The tail is cut into eight sub-ranges with one head each: a wave starts at head block % 8 (its XCD: one head word
// takes about 88 claims per microsecond, and thousands of waves drain the tail of a short launch at once) and moves on cyclically when a sub-range is
// exhausted.  A claim orders nothing (no wave reads what another wrote): one relaxed atomic add, no fence.  The index arithmetic is host-callable
// (tests/hostcheck/tile_queue_check.hip simulates the claims).
constexpr int TQ_HEADS = 8;
constexpr long long TQ_MAX_TILES = (1ll << 31) - 64;                     // the tail is indexed with 32-bit integers (the heads are int32)
struct TileQueue { long long n_static; int n_dyn, per_head; };            // tiles dealt statically, tiles in the tail, tiles per sub-range
O2345_HD TileQueue tile_queue_of(long long ntiles, int n_dyn) { return {ntiles - n_dyn, n_dyn, (n_dyn + TQ_HEADS - 1) / TQ_HEADS}; }
// share_shift: the tail is 1 / 2^share_shift of the list (0: everything); queued = false: the static schedule alone.  ntiles <= TQ_MAX_TILES.
O2345_HD TileQueue tile_queue_split(long long ntiles, long long total_waves, int share_shift, bool queued) {
    if (!queued) return {ntiles, 0, 0};
    long long ns = ntiles - (ntiles >> share_shift);
    ns -= ns % total_waves;
    return tile_queue_of(ntiles, (int)(ntiles - ns));
}
O2345_HD int tile_queue_lo(const TileQueue& q, int head) {                // first tile of a sub-range, relative to n_static; head == TQ_HEADS: the tail's end
    const long long lo = (long long)head * q.per_head;
    return lo < q.n_dyn ? (int)lo : q.n_dyn;
}
struct TileWalk { int head, left; };                                      // current head, heads not yet found exhausted
O2345_HD TileWalk tile_walk_begin(int block) { return {block & (TQ_HEADS - 1), TQ_HEADS}; }
// outcome of one claim (`claimed`: what the atomic add of C to heads[w.head] returned): the claim's first tile and `end`, or -1 after moving to the next head
O2345_HD long long tile_walk_take(const TileQueue& q, TileWalk& w, int claimed, int C, long long& end) {
    const long long t = (long long)tile_queue_lo(q, w.head) + claimed, hi = tile_queue_lo(q, w.head + 1);
    if (t < hi) {
        end = q.n_static + (t + C < hi ? t + C : hi);
        return q.n_static + t;
    }
    w.head = (w.head + 1) & (TQ_HEADS - 1);
    --w.left;
    return -1;
}

// The launch function behind o2345_color_points_{x3,mfma}[_q] (csrc/color_mfma.hip): the public entry points' arguments plus the queue, which must be zero
// when the kernel starts (the _q entry points clear it on the stream; o2345_render_rays hands out counters that its first kernel clears).
int color_points_launch(int x3, const float* blob, const float* vol_cl, const float* maskvol, int D, const float* cmaps, const float* proj,
                        const float* cam_pos, int V, int H, int W, const float* pts, const int32_t* index, const int32_t* n_dev, long long n,
                        const float* query_cam, const float* normals, float* out_rgb, uint8_t* out_nviews, unsigned long long* stats_dev, int32_t* tile_queue,
                        void* stream);

#if defined(__HIPCC__)
__device__ __forceinline__ TileSched tile_schedule_tiles(long long ntiles, int wave, int nwave) {
    return tile_schedule_at(ntiles, blockIdx.x, gridDim.x, wave, nwave);
}
__device__ __forceinline__ TileSched tile_schedule(long long n_units, int units_per_tile, int wave, int nwave) {
    return tile_schedule_tiles((n_units + units_per_tile - 1) / units_per_tile, wave, nwave);
}

// The tile loop of a kernel that takes a queue:
//     for (long long tile = tile_first<C>(cur, ts, q, heads); tile >= 0; tile = tile_next<C>(cur, tile, ntiles, heads, static_end))
// with q = tile_queue_split(ntiles, ...) and ts the static schedule over q.n_static tiles.  heads == nullptr: the static loop.  All of the state is
// wave-uniform, and what lives across a tile's body is kept small (these kernels have no scalar register to spare): the stride, the tail's length and the
// packed walk.  The rest is derived again from them at the end of each tile (static_end: see tile_next); the empty asm keeps the compiler from hoisting
// that out of the loop.
struct TileCursor { int stride, n_dyn, walk; long long claim_end; };      // stride == 0: the static share is done; walk = head | left << 4; claim_end: C > 1 only
template <int C>
__device__ __forceinline__ long long tile_claim(TileCursor& c, const TileQueue& q, int* heads) {
    c.stride = 0;
    TileWalk w{c.walk & 15, c.walk >> 4};
    long long first = -1;
    while (first < 0 && w.left > 0) {
        int t = 0;
        if (lane_id() == 0) t = __hip_atomic_fetch_add(heads + w.head, C, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        first = tile_walk_take(q, w, __builtin_amdgcn_readfirstlane(t), C, c.claim_end);
    }
    c.walk = w.head | w.left << 4;
    return first;
}
template <int C>
__device__ __forceinline__ long long tile_first(TileCursor& c, const TileSched& ts, const TileQueue& q, int* heads) {
    const TileWalk w = tile_walk_begin(blockIdx.x);
    c = TileCursor{(int)ts.stride, q.n_dyn, w.head | w.left << 4, 0};
    if (ts.first < ts.end) return ts.first;
    return heads ? tile_claim<C>(c, q, heads) : -1;
}
template <int C, class StaticEnd>           // static_end(n_static): this wave's TileSched::end of the static schedule over n_static tiles
__device__ __forceinline__ long long tile_next(TileCursor& c, long long tile, long long ntiles, int* heads, StaticEnd&& static_end) {
    asm volatile("" : "+s"(c.n_dyn));
    const TileQueue q = tile_queue_of(ntiles, c.n_dyn);
    if (c.stride) {
        tile += c.stride;
        if (tile < static_end(q.n_static)) return tile;
        if (!heads) return -1;
    } else if (C > 1 && tile + 1 < c.claim_end) {
        return tile + 1;
    }
    return tile_claim<C>(c, q, heads);
}
#endif

}  // namespace o2345
