// trees.hpp -- individual trees from a canopy band: tree tops by a variable-window local-maximum filter (lidR's
// locate_trees(lmf(ws))) and crown labels by seeded descent (in the manner of segment_trees(dalponte2016())).  The contract, for
// the device (csrc/trees.hip), the C-ABI's host twin (pcr_hip_trees_host) and the host engine (host/src/trees.h): all compile
// these lines with contraction off, and everything below is comparisons and integer arithmetic, so they agree bit for bit.
//
// Input   one Float32 band H, w x h, rows `stride` floats apart.  A cell whose value is not finite (NaN, +-Inf) is NO DATA, every
//         other cell a DATA CELL.  idx(r, c) = r * w + c; w * h < 2^31.
// Params  min_height (2.0f; finite), window_base (3.0f; finite, >= 0), window_slope (0.07f; finite, >= 0), max_radius_cells
//         (16; 1..32), min_crown_height (2.0f; finite), crown_ratio (0.45f; in [0, 1]), max_crown_radius (10.0f; > 0, +Inf: no
//         limit).  window_base + window_slope * height is lidR's window DIAMETER in map units; max_crown_radius is in map units.
//         cell = max(|cell_size_x|, |cell_size_y|), as in the ground filter.  The host computes once:
//           k = 0.5 / cell                                                          (refused unless finite)
//           M = -1 for +Inf, else (int64)min(floor((double)max_crown_radius / cell), 2^31 - 1)
// Order   a > b ("a beats b") when H[a] > H[b], or H[a] == H[b] and idx(a) < idx(b): plain binary32 comparisons (-0.0 == +0.0).
//         A strict total order on data cells: no parent chain can cycle.
// Window  of a data cell c: d = (double)window_base + (double)window_slope * (double)H[c] (two rounded binary64 operations),
//         rho = d * k; R(c) = max_radius_cells if rho >= max_radius_cells, 0 if !(rho >= 1), else (int)rho.  The disc of c is
//         the data cells at offsets dr*dr + dc*dc <= R*R, clipped to the image; best(c) is the greatest cell of the disc, c
//         included.
// Top     a data cell with H[c] >= min_height and best(c) == c.  Tops are numbered 1..T in increasing idx.
// Crown   set: the tops plus every data cell with H[c] >= min_crown_height.
// Parent  of a crown cell: (1) a top is its own; (2) else the greatest of its eight neighbours that are data cells and beat c;
//         (3) if there is none -- a local maximum that a taller cell of its window suppressed -- best(c) if that is not c, else c.
//         root(c) is the fixpoint of parent.
// Label   a crown cell carries id(root) when root is a top, and c == root or H[c] >= crown_ratio * H[root] (one binary32
//         multiplication, one comparison), and M < 0 or dr*dr + dc*dc <= M*M in 64-bit integers, (dr, dc) the offset from c to
//         its root.  Otherwise it carries none.
// Bands   tree_id = (float)id, tree_height = H[root] bit for bit; both 0x7FC00000 where there is no label.  An id above 2^24 is
//         not exact in Float32: cells of such trees are 0x7FC00000 in BOTH bands (id_exact); a table of more than 2^24 trees is
//         refused by the accessors above the C-ABI.
// Table   one row per top in id order: row, col, height = H[top], crown_cells = the number of cells whose label is the id (the
//         clamp above plays no part) -- a count of integer increments: any order gives the same bits.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define PCR_TREES_HD __host__ __device__ __forceinline__
#else
#define PCR_TREES_HD inline
#endif

namespace pcrhip {
namespace trees {

constexpr int kMaxRadius = 32;
constexpr int64_t kMaxExactId = (int64_t)1 << 24;

// what a launch (a host loop) is given besides the band
struct Consts {
    float min_height, window_base, window_slope;
    int max_radius;
    float min_crown_height, crown_ratio;
    double k;                        // 0.5 / cell
    int64_t M;                       // the crown radius in cells; -1: no limit
};

PCR_TREES_HD float nodata() {
    const uint32_t bits = 0x7FC00000u;
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}

PCR_TREES_HD bool is_data(float x) {
    uint32_t b;
    __builtin_memcpy(&b, &x, 4);
    return (b & 0x7F800000u) != 0x7F800000u;
}

// a beats b; both data cells
PCR_TREES_HD bool beats(float ha, int64_t ia, float hb, int64_t ib) { return ha > hb || (ha == hb && ia < ib); }

PCR_TREES_HD int radius(float h, const Consts& k) {
    const double d = (double)k.window_base + (double)k.window_slope * (double)h;
    const double rho = d * k.k;
    if (rho >= (double)k.max_radius) return k.max_radius;
    if (!(rho >= 1.0)) return 0;
    return (int)rho;
}

// the label conditions of crown cell (r, c) with value h whose root (rr, rc), value hr, is a top
PCR_TREES_HD bool labelled(float h, int r, int c, float hr, int rr, int rc, const Consts& k) {
    if (r == rr && c == rc) return true;
    const float bar = k.crown_ratio * hr;
    if (!(h >= bar)) return false;
    if (k.M < 0) return true;
    const int64_t dr = (int64_t)r - rr, dc = (int64_t)c - rc;
    return dr * dr + dc * dc <= k.M * k.M;
}

// whether a band can carry the id
PCR_TREES_HD bool id_exact(int64_t id) { return id <= kMaxExactId; }
// ... and what the id band holds for it
PCR_TREES_HD float id_value(int64_t id) { return id_exact(id) ? (float)id : nodata(); }

// k and M of the contract; cell = max(|cell_size_x|, |cell_size_y|)
inline double k_of(double cell) { return 0.5 / cell; }
inline int64_t M_of(float max_crown_radius, double cell) {
    if (max_crown_radius > 3.4028234663852886e38f) return -1;
    const double q = __builtin_floor((double)max_crown_radius / cell);
    return (int64_t)(q < 2147483647.0 ? q : 2147483647.0);
}

// ---- the host twin -----------------------------------------------------------------------------------------------------------
struct HostTable {
    std::vector<int32_t> row, col, crown_cells;
    std::vector<float> height;
};

// Both bands (height_dst may be null) and the table (may be null) of one band on the host.  Returns T.  Roots are resolved by
// walking with path compression; the discs are scanned only where the contract needs best(c).
inline int64_t host(const float* src, int w, int h, int64_t stride, const Consts& k, float* id_dst, int64_t id_stride,
                    float* height_dst, int64_t height_stride, HostTable* table) {
    const int64_t n = (int64_t)w * h;
    auto H = [&](int64_t i) { float x; std::memcpy(&x, src + (i / w) * stride + (i % w), 4); return x; };
    std::vector<int32_t> parent((size_t)n, -1), id((size_t)n, 0);
    int64_t T = 0;
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const int64_t i = (int64_t)r * w + c;
            const float hc = H(i);
            if (!is_data(hc)) continue;
            const int R = radius(hc, k);
            // the greatest neighbour that beats c
            int64_t nb = -1;
            float hn = 0.0f;
            for (int dr = -1; dr <= 1; ++dr)
                for (int dc = -1; dc <= 1; ++dc) {
                    if ((!dr && !dc) || r + dr < 0 || r + dr >= h || c + dc < 0 || c + dc >= w) continue;
                    const int64_t j = i + (int64_t)dr * w + dc;
                    const float x = H(j);
                    if (!is_data(x) || !beats(x, j, hc, i)) continue;
                    if (nb < 0 || beats(x, j, hn, nb)) { nb = j; hn = x; }
                }
            // best(c): a disc of R >= 2 holds the eight neighbours, so c is not its best when one of them beats it -- and
            // which cell is then never asked
            int64_t best = i;
            if (R < 2 || nb < 0) {
                float hb = hc;
                for (int dr = -R; dr <= R; ++dr)
                    for (int dc = -R; dc <= R; ++dc) {
                        if (dr * dr + dc * dc > R * R || r + dr < 0 || r + dr >= h || c + dc < 0 || c + dc >= w) continue;
                        const int64_t j = i + (int64_t)dr * w + dc;
                        const float x = H(j);
                        if (is_data(x) && beats(x, j, hb, best)) { best = j; hb = x; }
                    }
            } else {
                best = nb;
            }
            const bool top = hc >= k.min_height && best == i;
            if (top) {
                id[(size_t)i] = (int32_t)++T;
                parent[(size_t)i] = (int32_t)i;
            } else if (hc >= k.min_crown_height) {
                parent[(size_t)i] = (int32_t)(nb >= 0 ? nb : best);
            }
        }
    // roots
    for (int64_t i = 0; i < n; ++i) {
        if (parent[(size_t)i] < 0) continue;
        int64_t root = i;
        while (parent[(size_t)root] != root) root = parent[(size_t)root];
        for (int64_t j = i; j != root;) {
            const int64_t next = parent[(size_t)j];
            parent[(size_t)j] = (int32_t)root;
            j = next;
        }
    }
    if (table) {
        table->row.assign((size_t)T, 0);
        table->col.assign((size_t)T, 0);
        table->crown_cells.assign((size_t)T, 0);
        table->height.assign((size_t)T, 0.0f);
    }
    const float none = nodata();
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const int64_t i = (int64_t)r * w + c;
            float vid = none, vh = none;
            const int64_t root = parent[(size_t)i];
            if (root >= 0 && id[(size_t)root] > 0) {
                const int rr = (int)(root / w), rc = (int)(root % w);
                const float hr = H(root);
                if (labelled(H(i), r, c, hr, rr, rc, k)) {
                    const int64_t t = id[(size_t)root];
                    if (id_exact(t)) { vid = id_value(t); vh = hr; }
                    if (table) table->crown_cells[(size_t)t - 1] += 1;
                }
            }
            if (table && id[(size_t)i] > 0) {
                const size_t t = (size_t)id[(size_t)i] - 1;
                table->row[t] = r;
                table->col[t] = c;
                table->height[t] = H(i);
            }
            std::memcpy(id_dst + (int64_t)r * id_stride + c, &vid, 4);
            if (height_dst) std::memcpy(height_dst + (int64_t)r * height_stride + c, &vh, 4);
        }
    return T;
}

}  // namespace trees
}  // namespace pcrhip
