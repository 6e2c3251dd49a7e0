// What the two sparse-convolution units (sparse.hip: fp32 VALU form and the level construction; sparse_mfma.hip: matrix-core forms) share: the
// index grid of a level, the neighbour rule of the three convolution modes, and the list of channel pairs both entry points support.
#pragma once
#include "common.h"
#include <type_traits>

namespace o2345 {

// One level's dense index grid: the row of every cell, or -1 for an empty cell; x-major, as the rows of a level are numbered.
struct Lattice {
    int nx, ny, nz;   // cells per axis
    __host__ __device__ size_t cell(int x, int y, int z) const { return ((size_t)x * ny + y) * nz + z; }
    // the row of cell (x, y, z); -1 for an empty cell, for every cell outside the lattice (negative coordinates included), and when the caller does not
    // `want` the cell at all (one predicate in front of one load: a second test around the call would become a second branch)
    __device__ __forceinline__ int row_or_none(const int* grid, int x, int y, int z, bool want = true) const {
        return (want && x >= 0 && y >= 0 && z >= 0 && x < nx && y < ny && z < nz) ? grid[cell(x, y, z)] : -1;
    }
};

// The neighbour rule of the gather-form convolutions: the row of the input cell that offset k of the 3 x 3 x 3 kernel pairs with output cell
// (cx, cy, cz), or -1 when there is none (`live` false, pairing impossible, cell outside the input lattice, cell empty).
// k = (oz+1)*9 + (oy+1)*3 + (ox+1), o in {-1,0,1}^3 (x fastest, torchsparse odd-kernel order).
//   MODE 0 (stride 1)        cell + o       on the same level
//   MODE 1 (stride 2, down)  2 cell + o     on the finer level
//   MODE 2 (transposed, up)  (cell - o) / 2 on the coarser level, and only when all three of cell - o are even
// The bounds test is spelled out here and not taken from row_or_none: through the nested call the compiler allocates the registers of
// k_sparse_conv<48, 16, *> differently (volume front end); in this form every kernel keeps its register count.
template <int MODE>
__device__ __forceinline__ int neighbour_row(const int* __restrict__ in_grid, Lattice lin, int cx, int cy, int cz, int k, bool live = true) {
    const int ox = k % 3 - 1, oy = (k / 3) % 3 - 1, oz = k / 9 - 1;
    int nx, ny, nz;
    bool ok = live;
    if (MODE == 0) { nx = cx + ox; ny = cy + oy; nz = cz + oz; }
    else if (MODE == 1) { nx = 2 * cx + ox; ny = 2 * cy + oy; nz = 2 * cz + oz; }
    else {
        nx = cx - ox; ny = cy - oy; nz = cz - oz;
        ok = ok && !((nx | ny | nz) & 1);
        nx >>= 1; ny >>= 1; nz >>= 1;
    }
    ok = ok && nx >= 0 && ny >= 0 && nz >= 0 && nx < lin.nx && ny < lin.ny && nz < lin.nz;
    return ok ? in_grid[lin.cell(nx, ny, nz)] : -1;
}

// the (cin, cout) pairs of the two lod networks: o2345_sparse_conv3d and o2345_sparse_conv3d_x3 instantiate their kernels for exactly these
#define O2345_SPARSE_CHANNEL_PAIRS(X) X(32, 16) X(16, 16) X(16, 32) X(32, 32) X(32, 64) X(64, 64) X(64, 32) X(48, 16)

// calls f with the convolution mode (0, 1 or 2: the caller has checked it) as a compile-time constant
template <typename F>
auto with_conv_mode(int mode, F&& f) {
    if (mode == 0) return f(std::integral_constant<int, 0>{});
    if (mode == 1) return f(std::integral_constant<int, 1>{});
    return f(std::integral_constant<int, 2>{});
}

}  // namespace o2345
