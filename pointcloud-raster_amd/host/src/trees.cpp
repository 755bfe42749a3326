// trees.cpp -- segment_trees: tree tops and crown labels of a band, derived where its grid lives (pcr/core/trees.h).
#include "trees.h"

#include "buffer.h"

namespace pcr {
namespace detail {

// The table a pcr_hip_trees on `stream` left in `d_work` (without the centres): waits for the stream, twice.
Status tree_table_device(const float* d_src, int w, int h, int64_t stride, const void* d_work, size_t work_bytes, void* stream,
                         TreeTable* out) {
    *out = TreeTable();
    int64_t n = 0;
    Status s = hip_status(pcr_hip_trees_count(d_work, work_bytes, &n, nullptr, stream));
    if (!s.ok()) return s;
    if (n > tt::kMaxExactId) return tree_table_too_long(n);
    if (n == 0) return Status::success();
    const size_t rows = (size_t)n;
    Buffer d_table;                                               // [row][col][height][crown_cells], 4 bytes each
    if (!(s = d_table.allocate(4 * rows * 4, MemoryLocation::Device)).ok()) return s;
    int32_t* d = static_cast<int32_t*>(d_table.data());
    s = hip_status(pcr_hip_trees_table(d_src, w, h, stride, d_work, work_bytes, n, d, d + rows, reinterpret_cast<float*>(d + 2 * rows),
                                       d + 3 * rows, stream));
    out->row.resize(rows);
    out->col.resize(rows);
    out->height.resize(rows);
    out->crown_cells.resize(rows);
    if (s.ok()) s = hip_status(pcr_hip_memcpy_d2h(out->row.data(), d, rows * 4, stream));
    if (s.ok()) s = hip_status(pcr_hip_memcpy_d2h(out->col.data(), d + rows, rows * 4, stream));
    if (s.ok()) s = hip_status(pcr_hip_memcpy_d2h(out->height.data(), d + 2 * rows, rows * 4, stream));
    if (s.ok()) s = hip_status(pcr_hip_memcpy_d2h(out->crown_cells.data(), d + 3 * rows, rows * 4, stream));
    const Status ws = hip_status(pcr_hip_stream_synchronize(stream));             // (d_table is released behind the copies)
    if (s.ok()) s = ws;
    if (!s.ok()) *out = TreeTable();
    return s;
}

}  // namespace detail

std::unique_ptr<Grid> segment_trees(const Grid& grid, int band, const TreeSpec& spec, double cell_size_x, double cell_size_y,
                                    TreeTable* table, Status* status, void* stream) {
    auto fail = [&](const Status& s) {
        if (status) *status = s;
        return std::unique_ptr<Grid>();
    };
    auto refuse = [&](const std::string& msg) { return fail(Status::error(StatusCode::InvalidArgument, msg)); };
    if (table) *table = TreeTable();
    const std::string bad = detail::tree_spec_error(spec);
    if (!bad.empty()) return refuse("segment_trees: " + bad);
    if (!detail::tree_cell_sizes_ok(cell_size_x, cell_size_y)) return refuse("segment_trees: cell sizes must be finite and not zero");
    const int w = grid.cols(), h = grid.rows(), nb = grid.num_bands();
    if (w <= 0 || h <= 0 || nb <= 0) return refuse("segment_trees: empty grid");
    if (band < 0 || band >= nb) return refuse("segment_trees: band index outside the grid");
    if (grid.band_desc(band).dtype != DataType::Float32 || !grid.band_f32(band)) return refuse("segment_trees needs a Float32 band");
    if ((int64_t)w * h > 2147483647LL) return refuse("segment_trees: more than 2^31 - 1 cells");
    std::vector<BandDesc> descs(2);
    descs[0].name = "tree_id";
    descs[1].name = "tree_height";
    for (auto& d : descs) {
        d.dtype = DataType::Float32;
        d.is_state = false;
    }
    const MemoryLocation loc = grid.location();
    std::unique_ptr<Grid> out = Grid::create(w, h, descs, loc);
    if (!out) return fail(Status::error(StatusCode::OutOfMemory, "segment_trees: failed to allocate the derived grid"));
    if (grid.geometry()) (void)out->set_geometry(*grid.geometry());
    Status s = Status::success();
    TreeTable t;
    if (loc == MemoryLocation::Device) {
        const pcr_hip_tree_params p = detail::tree_params(spec, cell_size_x, cell_size_y);
        size_t bytes = 0;
        detail::Buffer work;
        s = detail::hip_status(pcr_hip_trees_work_bytes(w, h, &bytes));
        if (s.ok()) s = work.allocate(bytes, MemoryLocation::Device);
        if (s.ok())
            s = detail::hip_status(pcr_hip_trees(grid.band_f32(band), w, h, w, &p, out->band_f32(0), w, out->band_f32(1), w, work.data(),
                                                 work.bytes(), stream));
        if (s.ok() && table) s = detail::tree_table_device(grid.band_f32(band), w, h, w, work.data(), work.bytes(), stream, &t);
        const Status ws = detail::hip_status(pcr_hip_stream_synchronize(stream));
        if (s.ok()) s = ws;
    } else {
        s = detail::trees_host(grid.band_f32(band), w, h, w, detail::tree_consts(spec, cell_size_x, cell_size_y), out->band_f32(0), w,
                               out->band_f32(1), w, table ? &t : nullptr);
    }
    if (s.ok() && table) {
        detail::tree_centres(t, grid.geometry(), cell_size_x, cell_size_y);
        *table = std::move(t);
    }
    if (status) *status = s;
    if (!s.ok()) out.reset();
    return out;
}

}  // namespace pcr
