// polygonize.hpp -- the outlines of a label band's zones as rings of lattice corners (pcr_hip_polygonize_*, pcr::polygonize,
// Pipeline::polygonize): the inverse of rasterize.hpp.  One definition for the kernels (csrc/polygonize.hip), the C-ABI's host
// twin at the end of that file and the host layer (host/src/polygonize.cpp), compiled by all of them with contraction off.  The
// contract is written in include/pcr_hip.h ("polygonize") and DESIGN.md section 28.
//
//   zone     zonal::zone_of: a whole number in [1, 2^24]; NaN, +-Inf, 0, negatives, fractions, values above 2^24 and every cell
//            outside the band are no zone (0)
//   lattice  corner (i, j), i in 0..H, j in 0..W; cell (r, c) has the corners (r, c), (r, c+1), (r+1, c+1), (r+1, c)
//   edge     side s of a zone cell (0 top, 1 right, 2 bottom, 3 left) is a boundary edge when the cell across it has another
//            zone or none; it is directed with the cell on its right hand in (row-down, column-right) index space: top towards
//            +column, right towards +row, bottom towards -column, left towards -row.  Its slot is 4 * (r * W + c) + s.
//   next     F = the step of direction s, O = the step of direction (s + 3) % 4 (the outward normal); ahead = zone of cell + F,
//            diag = zone of cell + F + O.  ahead != z: (r, c, (s + 1) % 4), a right turn -- also at a saddle (diag == z), so
//            regions are 4-connected; else diag == z: (cell + F + O, (s + 3) % 4), a left turn; else (cell + F, s), straight on.
//            A permutation of each zone's boundary edges; its cycles are the rings.
//   corner   an edge whose predecessor has another side number: behind = zone of cell - F, bdiag = zone of cell - F + O; the
//            predecessor turned right when behind != z, left when bdiag == z, else it went straight.  A ring's vertices are the
//            start corners of its corner edges in cycle order, from the corner edge of smallest slot: the ring's key.
//   world    x = min_x + (double)j * cell_size_x, y = max_y + (double)i * cell_size_y: one rounded product, one rounded sum
#pragma once

#include "zonal.hpp"

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define PCR_PG_HD __host__ __device__ __forceinline__
#else
#define PCR_PG_HD inline
#endif

namespace pcrhip {
namespace polygonize {

constexpr int64_t kMaxCells = ((int64_t)1 << 30) - 1;          // 4 slots a cell below the sentinel
constexpr uint32_t kNone = 0xFFFFFFFFu;                         // no slot, no edge

// the step of direction s: 0 = +column, 1 = +row, 2 = -column, 3 = -row
PCR_PG_HD int step_r(int s) { return s == 1 ? 1 : s == 3 ? -1 : 0; }
PCR_PG_HD int step_c(int s) { return s == 0 ? 1 : s == 2 ? -1 : 0; }

// The zones of one band.
struct Band {
    const float* data;
    int w, h;
    int64_t stride;
    PCR_PG_HD uint32_t zone(int r, int c) const {
        if (r < 0 || r >= h || c < 0 || c >= w) return 0u;
        return zonal::zone_of(data[(int64_t)r * stride + c]);
    }
};

// The sides of zone cell (r, c) that are boundary edges: bit s.
PCR_PG_HD unsigned sides_of(const Band& b, int r, int c, uint32_t z) {
    unsigned m = 0;
    for (int s = 0; s < 4; ++s) {
        const int o = (s + 3) & 3;
        if (b.zone(r + step_r(o), c + step_c(o)) != z) m |= 1u << s;
    }
    return m;
}

// The successor of boundary edge (r, c, s) of zone z.
PCR_PG_HD void successor(const Band& b, int r, int c, int s, uint32_t z, int& nr, int& nc, int& ns) {
    const int o = (s + 3) & 3;
    const int fr = step_r(s), fc = step_c(s);
    if (b.zone(r + fr, c + fc) != z) {
        nr = r; nc = c; ns = (s + 1) & 3;
    } else if (b.zone(r + fr + step_r(o), c + fc + step_c(o)) == z) {
        nr = r + fr + step_r(o); nc = c + fc + step_c(o); ns = o;
    } else {
        nr = r + fr; nc = c + fc; ns = s;
    }
}

// Whether boundary edge (r, c, s) of zone z is a corner edge.
PCR_PG_HD bool is_corner(const Band& b, int r, int c, int s, uint32_t z) {
    const int o = (s + 3) & 3;
    const int br = r - step_r(s), bc = c - step_c(s);
    return b.zone(br, bc) != z || b.zone(br + step_r(o), bc + step_c(o)) == z;
}

// The start corner of edge (r, c, s).
PCR_PG_HD int corner_row(int r, int s) { return r + (s >= 2 ? 1 : 0); }
PCR_PG_HD int corner_col(int c, int s) { return c + (s == 1 || s == 2 ? 1 : 0); }

// The world coordinates of lattice corner (i, j).
PCR_PG_HD double world_x(double min_x, double cell_size_x, int j) {
    const double off = (double)j * cell_size_x;
    return min_x + off;
}
PCR_PG_HD double world_y(double max_y, double cell_size_y, int i) {
    const double off = (double)i * cell_size_y;
    return max_y + off;
}

// ---- the host twin: one thread, slots in ascending order, every unvisited corner edge's cycle walked with successor() -- a
// sequential trace, where the kernels double pointers.  The rings come out by ascending key.
struct HostRings {
    int64_t edges = 0;
    std::vector<uint32_t> ring_zone;         // R
    std::vector<int64_t> ring_offset;        // R + 1
    std::vector<int32_t> vertex_row, vertex_col;
};
inline void host(const Band& b, HostRings* out) {
    out->edges = 0;
    out->ring_zone.clear();
    out->ring_offset.assign(1, 0);
    out->vertex_row.clear();
    out->vertex_col.clear();
    std::vector<uint8_t> seen((size_t)b.w * (size_t)b.h, 0);         // bit s: the edge's ring is traced
    for (int r = 0; r < b.h; ++r)
        for (int c = 0; c < b.w; ++c) {
            const uint32_t z = b.zone(r, c);
            if (z == 0u) continue;
            const unsigned m = sides_of(b, r, c, z);
            out->edges += __builtin_popcount(m);
            for (int s = 0; s < 4; ++s) {
                if (!((m >> s) & 1u) || ((seen[(size_t)r * b.w + c] >> s) & 1u) || !is_corner(b, r, c, s, z)) continue;
                int er = r, ec = c, es = s;
                do {
                    seen[(size_t)er * b.w + ec] |= (uint8_t)(1u << es);
                    if (is_corner(b, er, ec, es, z)) {
                        out->vertex_row.push_back(corner_row(er, es));
                        out->vertex_col.push_back(corner_col(ec, es));
                    }
                    int nr, nc, ns;
                    successor(b, er, ec, es, z, nr, nc, ns);
                    er = nr; ec = nc; es = ns;
                } while (!(er == r && ec == c && es == s));
                out->ring_zone.push_back(z);
                out->ring_offset.push_back((int64_t)out->vertex_row.size());
            }
        }
}

}  // namespace polygonize
}  // namespace pcrhip
