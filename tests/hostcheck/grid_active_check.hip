// TEST-ONLY stand-alone host program: the activity rule of the sparse lattice evaluation (one-2-3-45_amd/csrc/geom_math.h: grid_point_active,
// grid_tile_active -- the source the pre-pass kernel of csrc/sdf_mlp_x3.hip executes) against brute force over trilinear_ref_taps.
// Prints one line per (R, D, mask) and exits non-zero on the first kind of mismatch.  Run by tests/test_grid_active_cpu.py.
#include "../../one-2-3-45_amd/csrc/geom_math.h"

#include <random>
#include <string>
#include <vector>

using namespace o2345;
namespace o2345 { void set_error(const char*, ...) {} }

// `ok && any corner kept`, the corners looped here, the slot decoded with 64-bit arithmetic
static bool brute_point(long long slot, int R, int D, const std::vector<float>& mask) {
    const long long iz = slot % R, iy = (slot / R) % R, ix = slot / ((long long)R * R);
    const Taps3D tp = trilinear_ref_taps(lin11((int)ix, R), lin11((int)iy, R), lin11((int)iz, R), D);
    int kept = 0;
    for (int c = 0; c < 8; ++c) kept += mask[((size_t)tp.ix[c >> 2] * D + tp.iy[(c >> 1) & 1]) * D + tp.iz[c & 1]] != 0.f;
    return tp.ok && kept > 0;
}

static int check(int R, int D, const char* name, const std::vector<float>& mask) {
    const long long n = (long long)R * R * R, ntiles = (n + 31) / 32;
    std::vector<char> expect(n);
    long long active = 0, bad_point = 0, bad_zero = 0, bad_tile = 0, active_tiles = 0, partial = 0, straddling = 0;
    for (long long s = 0; s < n; ++s) {
        expect[s] = brute_point(s, R, D, mask);
        active += expect[s];
        bad_point += grid_point_active(s, R, D, mask.data()) != (bool)expect[s];
        const long long iz = s % R, iy = (s / R) % R, ix = s / ((long long)R * R);
        if (ix == 0 || iy == 0 || iz == 0) bad_zero += grid_point_active(s, R, D, mask.data());      // `ok` is false at index 0 of any axis
    }
    for (long long t = 0; t < ntiles; ++t) {
        const long long lo = t * 32, hi = lo + 32 < n ? lo + 32 : n;
        bool any = false;
        for (long long s = lo; s < hi; ++s) any |= (bool)expect[s];
        bad_tile += grid_tile_active(t, R, D, mask.data()) != any;
        active_tiles += any;
        partial += hi - lo < 32;
        straddling += lo / R != (hi - 1) / R;
    }
    printf("R %d D %d mask %-12s points %lld active %lld tiles %lld active %lld partial %lld straddling %lld | mismatches: point %lld index0 %lld tile %lld\n", R, D,
           name, n, active, ntiles, active_tiles, partial, straddling, bad_point, bad_zero, bad_tile);
    int rc = (bad_point || bad_zero || bad_tile) ? 1 : 0;
    const std::string m(name);
    if (m == "empty" && (active || active_tiles)) { printf("  an empty mask must leave nothing active\n"); rc = 1; }
    if (m == "full" && active != (long long)(R - 1) * (R - 1) * (R - 1)) { printf("  a full mask must activate every point off the index-0 faces\n"); rc = 1; }
    // the lattice's last point sits on voxel D-1 with `ok` set; voxel 0 is a corner of lattice index 1 once the lattice is finer than the volume
    if ((m == "last" || (m == "first" && R > D)) && active == 0) { printf("  a kept corner voxel must activate the points around it\n"); rc = 1; }
    return rc;
}

int main() {
    const int cases[][2] = {{2, 2}, {32, 32}, {33, 16}, {40, 24}, {64, 16}};
    int rc = 0;
    for (const auto& c : cases) {
        const int R = c[0], D = c[1];
        const size_t nv = (size_t)D * D * D;
        std::vector<float> empty(nv, 0.f), full(nv, 1.f), first(nv, 0.f), last(nv, 0.f), rnd(nv);
        first[0] = 1.f;
        last[nv - 1] = 1.f;
        std::mt19937 gen(1234u + 100u * R + D);
        for (auto& v : rnd) v = (gen() % 100u) < 30u ? 1.f : 0.f;
        rc |= check(R, D, "empty", empty);
        rc |= check(R, D, "full", full);
        rc |= check(R, D, "first", first);
        rc |= check(R, D, "last", last);
        rc |= check(R, D, "random30", rnd);
    }
    printf(rc ? "FAILED\n" : "OK\n");
    return rc;
}
