// The grid object of a target mesh (built by mesh_distance.hip, walked by its query and by mesh_intersect.hip): its one layout, and the limit on its cells.
#pragma once
#include "mesh_common.h"
#include "mesh_distance_math.h"

namespace o2345 {

constexpr long long MD_MAX_CELLS = 1ll << 24;

// the grid object: head (128 bytes), then cell_start [max_cells + 1], then the entries
struct MdGridObject {
    MdGridHead* head;
    int *cell_start, *entries;
};

inline size_t md_grid_object(void* grid, long long max_cells, long long n_entries, MdGridObject& g) {
    Carver w(grid);
    g.head = w.take_bytes<MdGridHead>(128);
    g.cell_start = w.take<int>(max_cells + 1);
    g.entries = w.take<int>(n_entries);
    return w.bytes();
}

}  // namespace o2345
