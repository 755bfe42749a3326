// pcr/core/trees.h -- individual trees from a canopy band, done where the grid lives: tree tops by a variable-window
// local-maximum filter (lidR's locate_trees(lmf(ws)), PDAL's filters.litree) and crown labels by a seeded descent (in the manner
// of lidR's segment_trees(dalponte2016())).  Not in the reference.
//
// The contract, one definition for host and device (csrc/trees.hpp, include/pcr_hip.h: pcr_hip_trees).  A cell of the band H
// that is not finite is no data, every other a data cell; idx(r, c) = r * w + c.  cell = max(|cell_size_x|, |cell_size_y|),
// k = 0.5 / cell, M = -1 for max_crown_radius = +Inf, else (int64)min(floor((double)max_crown_radius / cell), 2^31 - 1).
//   order    a beats b when H[a] > H[b], or H[a] == H[b] and idx(a) < idx(b): a strict total order, no parent chain cycles
//   window   d = (double)window_base + (double)window_slope * (double)H[c] (lidR's window DIAMETER in map units; two rounded
//            operations), rho = d * k, R(c) = max_radius_cells if rho >= max_radius_cells, 0 if !(rho >= 1), else (int)rho.
//            The disc of c: the data cells at dr*dr + dc*dc <= R*R inside the image; best(c): its greatest cell, c included
//   top      a data cell with H[c] >= min_height and best(c) == c; tops are numbered 1..T in increasing idx
//   crown    set: the tops and every data cell with H[c] >= min_crown_height
//   parent   of a crown cell: a top is its own; else the greatest of its eight neighbours that are data cells and beat c; if
//            there is none (a local maximum a taller cell of its window suppressed) best(c) when that is not c, else c.
//            root(c) is the fixpoint of parent
//   label    id(root) when root is a top, and c == root or H[c] >= crown_ratio * H[root] (one binary32 multiplication), and
//            M < 0 or dr*dr + dc*dc <= M*M in 64-bit integers, (dr, dc) the offset from c to its root; else none
//   bands    tree_id = (float)id, tree_height = H[root] bit for bit, both 0x7FC00000 without a label.  Ids above 2^24 are not
//            exact in Float32: cells of such trees are NaN in both bands, and the table of a band with more than 2^24 trees is
//            refused (OutOfRange)
//   table    per top in id order: row, col, x, y (the cell centre), height = H[top], crown_cells = the cells that carry the
//            id: crown area is crown_cells * |cell_size_x * cell_size_y|
// Everything is comparisons and integer arithmetic: the result does not depend on threads, tiles or the order of atomics, and
// device and host agree bit for bit.  PipelineConfig::trees appends such bands at finalize().  "average" overview levels of an
// id band are not meaningful (like those of an aspect band): read level 0, or write "nearest" overviews.
#pragma once

#include "pcr/core/grid.h"
#include "pcr/core/types.h"

#include <cstdint>
#include <limits>
#include <memory>
#include <vector>

namespace pcr {

struct TreeSpec {
    float min_height = 2.0f;          // finite: a top is at least this high
    float window_base = 3.0f;         // finite, >= 0: window diameter ws(h) = window_base + window_slope * h, map units
    float window_slope = 0.07f;       // finite, >= 0
    int max_radius_cells = 16;        // 1..32: the window radius never exceeds this many cells
    float min_crown_height = 2.0f;    // finite: lower cells belong to no crown
    float crown_ratio = 0.45f;        // in [0, 1]: a crown cell is at least this share of its top's height
    float max_crown_radius = 10.0f;   // > 0, map units; +Inf: no limit
};

/// One row per tree, in id order (ids are 1..size()).
struct TreeTable {
    std::vector<int32_t> row, col;
    std::vector<double> x, y;         // the cell centre: by the grid's geometry when it has one, else min_x = 0, max_y = 0
    std::vector<float> height;
    std::vector<int32_t> crown_cells;
    size_t size() const { return row.size(); }
};

/// A new grid at `grid`'s location with the bands "tree_id" and "tree_height" of band `band` of `grid`, and (when asked) the
/// table.  Host grids: the host twin.  Device grids: pcr_hip_trees on `stream`, synchronised once, for the table.  nullptr and
/// `status` on failure: InvalidArgument for a band index outside the grid, a band that is not Float32, a spec outside its
/// ranges, a cell size that is zero or not finite or more than 2^31 - 1 cells; OutOfRange for a table of more than 2^24 trees.
std::unique_ptr<Grid> segment_trees(const Grid& grid, int band, const TreeSpec& spec = TreeSpec(), double cell_size_x = 1.0,
                                    double cell_size_y = -1.0, TreeTable* table = nullptr, Status* status = nullptr,
                                    void* stream = nullptr);

}  // namespace pcr
