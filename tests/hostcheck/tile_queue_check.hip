// TEST-ONLY stand-alone host program: the index arithmetic of the tile queue (one-2-3-45_amd/csrc/common.h: tile_schedule_at, tile_schedule_flat_at,
// tile_queue_split, tile_queue_lo, tile_walk_begin, tile_walk_take -- the functions the device loop tile_first / tile_next / tile_claim is made of).
// For many (n_tiles, grid, waves per block, share, tiles per claim) it walks every wave's static share, then lets the waves claim from eight host-side
// heads in a random interleaving, and checks that every tile of [0, n_tiles) was taken exactly once.  Run by tests/test_tile_queue_cpu.py.
#include "../../one-2-3-45_amd/csrc/common.h"

#include <random>
#include <vector>

using namespace o2345;
namespace o2345 { void set_error(const char*, ...) {} }

struct Result { long long cases = 0, bad = 0, small = 0, empty = 0, idle_heads = 0, claims = 0, queued_tiles = 0; };

static bool one_case(long long ntiles, int grid, int nwave, int shift, int C, bool flat, bool queued, std::mt19937& gen, Result& r) {
    const long long total_waves = (long long)grid * nwave;
    const TileQueue q = tile_queue_split(ntiles, total_waves, shift, queued);
    std::vector<int> taken((size_t)ntiles, 0);
    bool ok = queued ? q.n_static >= 0 && q.n_dyn >= 0 && q.n_static + q.n_dyn == ntiles && q.n_static % total_waves == 0 && (shift || q.n_static == 0)
                     : q.n_static == ntiles && q.n_dyn == 0;
    // the eight sub-ranges tile the tail in order
    ok = ok && tile_queue_lo(q, 0) == 0 && tile_queue_lo(q, TQ_HEADS) == q.n_dyn;
    for (int h = 0; h < TQ_HEADS; ++h) {
        ok = ok && tile_queue_lo(q, h) <= tile_queue_lo(q, h + 1);
        r.idle_heads += queued && tile_queue_lo(q, h) == tile_queue_lo(q, h + 1);
    }
    // static shares: every wave the same number of tiles
    long long share0 = -1;
    for (int b = 0; b < grid; ++b)
        for (int w = 0; w < nwave; ++w) {
            const TileSched ts = flat ? tile_schedule_flat_at(q.n_static, b, grid, w, nwave) : tile_schedule_at(q.n_static, b, grid, w, nwave);
            long long cnt = 0;
            for (long long t = ts.first; t < ts.end; t += ts.stride, ++cnt) {
                if (t < 0 || t >= ntiles) return false;
                ++taken[(size_t)t];
            }
            if (queued) {
                if (share0 < 0) share0 = cnt;
                ok = ok && cnt == share0;
            }
        }
    // the tail: waves claim in a random interleaving (each step: one wave does one atomic add and looks at what it got)
    if (queued) {
        int heads[TQ_HEADS] = {0};
        std::vector<TileWalk> walk;
        std::vector<int> active;
        for (int b = 0; b < grid; ++b)
            for (int w = 0; w < nwave; ++w) {
                walk.push_back(tile_walk_begin(b));
                ok = ok && walk.back().head == (b & 7) && walk.back().left == TQ_HEADS;
                active.push_back((int)walk.size() - 1);
            }
        while (!active.empty()) {
            const size_t pick = gen() % active.size();
            TileWalk& w = walk[(size_t)active[pick]];
            const int claimed = heads[w.head];
            heads[w.head] += C;
            ++r.claims;
            long long end = -1;
            const long long first = tile_walk_take(q, w, claimed, C, end);
            if (first >= 0) {
                if (first < q.n_static || end > ntiles || end <= first || end - first > C) return false;
                for (long long t = first; t < end; ++t) ++taken[(size_t)t];
                r.queued_tiles += end - first;
            } else if (w.left == 0) {
                active[pick] = active.back();
                active.pop_back();
            }
        }
        for (int h = 0; h < TQ_HEADS; ++h) ok = ok && heads[h] >= tile_queue_lo(q, h + 1) - tile_queue_lo(q, h);     // every sub-range was drained
    }
    for (long long t = 0; t < ntiles; ++t) ok = ok && taken[(size_t)t] == 1;
    ++r.cases;
    r.small += ntiles < 8;
    r.empty += ntiles == 0;
    return ok;
}

int main() {
    std::mt19937 gen(20240611u);
    Result r;
    const int grids[] = {1, 2, 7, 8, 9, 16, 24, 31, 64, 255, 256};
    const int waves[] = {1, 8, 12};
    const int shifts[] = {0, 2, 3, 4};
    std::vector<long long> sizes = {0, 1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65};
    for (int i = 0; i < 12; ++i) sizes.push_back(gen() % 40000u);
    for (const int g : grids)
        for (const int nw : waves) {
            std::vector<long long> ns = sizes;
            const long long W = (long long)g * nw;
            for (const long long k : {W - 1, W, W + 1, 8 * W - 1, 8 * W, 8 * W + 1, 9 * W + 5, 40 * W + 3}) ns.push_back(k);
            for (const long long n : ns)
                for (const int sh : shifts)
                    for (const int C : {1, 2, 3})
                        for (const int flat : {0, 1}) {
                            if (C == 3 && (n > 4000 || sh != 3)) continue;            // a third claim size on the short lists only
                            if (!one_case(n, g, nw, sh, C, flat != 0, true, gen, r)) {
                                printf("MISMATCH n_tiles %lld grid %d waves %d shift %d C %d flat %d\n", n, g, nw, sh, C, flat);
                                ++r.bad;
                            }
                        }
            for (const long long n : ns)                                               // no queue: the static schedule covers the list alone
                for (const int flat : {0, 1})
                    if (!one_case(n, g, nw, 3, 1, flat != 0, false, gen, r)) {
                        printf("MISMATCH (static) n_tiles %lld grid %d waves %d flat %d\n", n, g, nw, flat);
                        ++r.bad;
                    }
        }
    printf("cases %lld empty %lld below8 %lld idle_heads %lld claims %lld queued_tiles %lld mismatches %lld\n", r.cases, r.empty, r.small, r.idle_heads, r.claims,
           r.queued_tiles, r.bad);
    printf(r.bad ? "FAILED\n" : "OK\n");
    return r.bad ? 1 : 0;
}
