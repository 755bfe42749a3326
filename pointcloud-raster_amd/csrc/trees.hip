// trees.hip -- pcr_hip_trees: tree tops and crown labels of one canopy band (the contract: trees.hpp), and what goes with it:
// the work area's size, the tree count, the table, the host twin.
//
// The work area holds, per cell, root (int32: the parent, later the root; -1: no crown cell), top (int32: 0 / 1, later the
// id) and count (int32: crown cells, at the root's cell), a partial sum per 1024 cells, and a head of 64 words: T and one
// "changed" word per jumping round.  Seven kinds of launch, all on the caller's stream, none waited for:
//   1  k_tree_cells   one workgroup of 256 lanes per 64 x 32 tile, staged in LDS with a 1-cell apron as in terrain.hip; a lane
//                     owns four cells of two rows.  Per cell: the greatest of the eight neighbours that beats it (the parent
//                     by step 2), the window radius R, and everything R <= 1 decides on the spot (its disc lies inside the
//                     3 x 3 window).  With R >= 2 the disc holds the eight neighbours: a cell one of them beats is no top and
//                     never asks for best(c); only a 3 x 3 local maximum is left PENDING.  Almost every cell ends here.
//   2  k_tree_disc    a wave reads 64 consecutive root words, ballots the pending ones and takes them in turn: the disc's cells
//                     are spread over the 64 lanes (R <= 3: one cell per lane in one step; beyond: a row per step, a lane per
//                     column, the loads of a row one coalesced segment from L2), each lane keeps its best, six xor-shuffles
//                     reduce them under the order.  Lane 0 stores the verdict.
//   3  k_tree_count, k_tree_scan, k_tree_number   tops per 1024 cells, an exclusive scan of those sums by one workgroup (T stays
//                     in the head), ids in idx order written over the flags.
//   4  k_tree_jump    ceil(log2(w h)) + 1 rounds of root[c] = root[root[c]], in place, with relaxed agent-scope loads and
//                     stores: whatever version of root[p] a lane reads is an ancestor of p, pointers only move towards the
//                     root, only lane c stores root[c], so a round covers at least twice the distance of the one before and
//                     the fixpoint is unique.  A round that changes a pointer sets its word of the head; the next round
//                     returns at once when the word of the one before is clear.
//   5  k_tree_label   a lane per four cells of a row: the label conditions, both bands (16-byte non-temporal stores where
//                     the rows allow), one vector atomic add per labelled cell on count[root].
//   6  k_tree_table   (pcr_hip_trees_table) a lane per cell, the tops store row id - 1.
// No kernel uses scratch.  Measured: profiles/trees.md.
#include "band_pass.hpp"
#include "trees.hpp"

#include <algorithm>

namespace pcrhip {
namespace {

using namespace trees;
using band::load_quad;

constexpr int kTileW = 64, kTileH = 32;
constexpr int kPitch = kTileW + 8;                               // image column c0 - 1 is LDS column 3: the body's quads stay aligned
constexpr int kRows = kTileH + 2;
constexpr int kPending = -2;
constexpr int kChunk = 1024;                                     // cells per partial sum
constexpr int kHeadWords = 64;
constexpr int kMaxRounds = 40;

struct Work {
    uint32_t* head;                  // [0] T, [8 + round] changed
    int32_t* root;
    int32_t* top;
    int32_t* count;
    int32_t* partial;
    int chunks;
};
constexpr int kChangedAt = 8;

size_t quads(int64_t n) { return (size_t)((n + 3) & ~(int64_t)3); }
size_t work_bytes_of(int width, int height) {
    const int64_t n = (int64_t)width * height;
    return 16 + (size_t)kHeadWords * 4 + 3 * quads(n) * 4 + quads((n + kChunk - 1) / kChunk) * 4;
}
Work carve(void* d_work, int width, int height) {
    const int64_t n = (int64_t)width * height;
    Work k;
    k.head = reinterpret_cast<uint32_t*>((reinterpret_cast<uintptr_t>(d_work) + 15) & ~(uintptr_t)15);
    k.root = reinterpret_cast<int32_t*>(k.head + kHeadWords);
    k.top = k.root + quads(n);
    k.count = k.top + quads(n);
    k.partial = k.count + quads(n);
    k.chunks = (int)((n + kChunk - 1) / kChunk);
    return k;
}

struct TreeArgs {
    const float* src;
    int w, h;
    int64_t stride;
    int n;                           // w * h
    Work work;
    Consts k;
    float* id_dst;
    float* height_dst;               // null: not asked for
    int64_t id_stride, height_stride;
    int wvec;                        // w % 4 == 0: the work area's rows start on 16 bytes
    int dvec;                        // the rows of both bands start on 16 bytes
};

__device__ __forceinline__ void store4(int32_t* p, int i, int valid, int a, int b, int c, int d, int wvec) {
    if (wvec && valid == 4) {
        *reinterpret_cast<int4*>(p + i) = make_int4(a, b, c, d);
    } else {
        p[i] = a;
        if (valid > 1) p[i + 1] = b;
        if (valid > 2) p[i + 2] = c;
        if (valid > 3) p[i + 3] = d;
    }
}

// ---- 1
template <bool VEC>
__global__ __launch_bounds__(256) void k_tree_cells(const TreeArgs a) {
    __shared__ __attribute__((aligned(16))) float tile[kRows * kPitch];
    const int tid = threadIdx.x;
    const int lx = tid & 15, ly = tid >> 4;
    const int c0 = blockIdx.x * kTileW, r0 = blockIdx.y * kTileH;
    const int c = c0 + 4 * lx;

    // the body, a quad per lane and tile half ...
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = r0 + ly + 16 * p;
        const float4 x = load_quad<VEC>(r < a.h ? a.src + (int64_t)r * a.stride : nullptr, c, a.w);
        *reinterpret_cast<float4*>(&tile[(1 + ly + 16 * p) * kPitch + 4 + 4 * lx]) = x;
    }
    // ... and the apron: lanes 0..31 the quads of the rows above and below, lanes 32..99 the cells left and right
    if (tid < 32) {
        const int below = tid >> 4, gc = c0 + 4 * (tid & 15);
        const int r = below ? r0 + kTileH : r0 - 1;
        const float4 x = load_quad<VEC>(r >= 0 && r < a.h ? a.src + (int64_t)r * a.stride : nullptr, gc, a.w);
        *reinterpret_cast<float4*>(&tile[(below ? kRows - 1 : 0) * kPitch + 4 + 4 * (tid & 15)]) = x;
    } else if (tid < 32 + 2 * kRows) {
        const int j = tid - 32, right = j & 1, lr = j >> 1;
        const int r = r0 - 1 + lr, gc = right ? c0 + kTileW : c0 - 1;
        float x = nodata();
        if (r >= 0 && r < a.h && gc >= 0 && gc < a.w) x = a.src[(int64_t)r * a.stride + gc];
        tile[lr * kPitch + (right ? 4 + kTileW : 3)] = x;
    }
    __syncthreads();

    if (c >= a.w) return;
    const int valid = min(4, a.w - c);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = r0 + ly + 16 * p;
        if (r >= a.h) continue;
        const float* t = &tile[(ly + 16 * p) * kPitch + 3 + 4 * lx];      // the window's first cell of the quad's first cell
        float v[3][6];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float4 m = *reinterpret_cast<const float4*>(t + d * kPitch + 1);
            v[d][0] = t[d * kPitch];
            v[d][1] = m.x; v[d][2] = m.y; v[d][3] = m.z; v[d][4] = m.w;
            v[d][5] = t[d * kPitch + 5];
        }
        int pr[4], tp[4];
        const int i0 = r * a.w + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float hc = v[1][j + 1];
            const int i = i0 + j;
            pr[j] = -1;
            tp[j] = 0;
            if (!is_data(hc)) continue;                          // (a cell right of the image is NaN in the tile)
            // the greatest neighbour that beats c: in idx order, so that among equals the first stays
            int nb = -1;
            float hn = 0.0f;
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                if (q == 4) continue;
                const float x = v[q / 3][j + q % 3];
                const bool wins = q < 4 ? x >= hc : x > hc;
                if (is_data(x) && wins && (nb < 0 || x > hn)) { nb = i + (q / 3 - 1) * a.w + (q % 3 - 1); hn = x; }
            }
            const int R = radius(hc, a.k);
            const bool crown = hc >= a.k.min_crown_height;
            if (R >= 2) {
                pr[j] = nb >= 0 ? (crown ? nb : -1) : kPending;
                continue;
            }
            // R <= 1: the disc is c alone, or c and its four edge neighbours
            bool best_is_c = true;
            if (R == 1) {
                const float up = v[0][j + 1], left = v[1][j], right = v[1][j + 2], down = v[2][j + 1];
                best_is_c = !(is_data(up) && up >= hc) && !(is_data(left) && left >= hc) && !(is_data(right) && right > hc) &&
                            !(is_data(down) && down > hc);
            }
            if (hc >= a.k.min_height && best_is_c) {
                pr[j] = i;
                tp[j] = 1;
            } else if (crown) {
                pr[j] = nb >= 0 ? nb : i;                        // (no neighbour beats c: nor does a cell of its disc)
            }
        }
        store4(a.work.root, i0, valid, pr[0], pr[1], pr[2], pr[3], a.wvec);
        store4(a.work.top, i0, valid, tp[0], tp[1], tp[2], tp[3], a.wvec);
        store4(a.work.count, i0, valid, 0, 0, 0, 0, a.wvec);
    }
}

// ---- 2
__global__ __launch_bounds__(256) void k_tree_disc(const TreeArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    const int64_t mine = base + lane;
    const bool pending = mine < a.n && a.work.root[mine] == kPending;
    unsigned long long todo = __ballot(pending);
    while (todo) {
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int j = (int)(base + b);
        const int r = j / a.w, c = j - r * a.w;
        const float hc = a.src[(int64_t)r * a.stride + c];
        const int R = radius(hc, a.k);
        float hb = hc;
        int bi = j;
        const int D = 2 * R + 1;
        if (D * D <= 64) {
            if (lane < D * D) {
                const int dr = lane / D - R, dc = lane - (lane / D) * D - R;
                const int rr = r + dr, cc = c + dc;
                if (dr * dr + dc * dc <= R * R && rr >= 0 && rr < a.h && cc >= 0 && cc < a.w) {
                    const float x = a.src[(int64_t)rr * a.stride + cc];
                    const int i = rr * a.w + cc;
                    if (is_data(x) && beats(x, i, hb, bi)) { hb = x; bi = i; }
                }
            }
        } else {
            for (int dr = -R; dr <= R; ++dr) {
                const int rr = r + dr;
                if (rr < 0 || rr >= a.h) continue;
                const float* row = a.src + (int64_t)rr * a.stride;
                for (int dc = lane - R; dc <= R; dc += 64) {
                    const int cc = c + dc;
                    if (dr * dr + dc * dc > R * R || cc < 0 || cc >= a.w) continue;
                    const float x = row[cc];
                    const int i = rr * a.w + cc;
                    if (is_data(x) && beats(x, i, hb, bi)) { hb = x; bi = i; }
                }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ho = __shfl_xor(hb, off);
            const int io = __shfl_xor(bi, off);
            if (beats(ho, io, hb, bi)) { hb = ho; bi = io; }
        }
        if (lane == 0) {
            const bool top = hc >= a.k.min_height && bi == j;
            a.work.root[j] = top ? j : hc >= a.k.min_crown_height ? bi : -1;
            a.work.top[j] = top ? 1 : 0;
        }
    }
}

// ---- 3
// v's exclusive prefix over the workgroup's 256 lanes; total: the sum of all
__device__ __forceinline__ int block_scan(int v, int* lds, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(s, off);
        if (lane >= off) s += o;
    }
    __syncthreads();                                             // (lds may still be read from the call before)
    if (lane == 63) lds[wave] = s;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = lds[k];
        if (k < wave) before += x;
        all += x;
    }
    *total = all;
    return before + s - v;
}

__device__ __forceinline__ void load_flags(const int32_t* top, int64_t i, int n, int f[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = i + k < n ? top[i + k] : 0;
}

__global__ __launch_bounds__(256) void k_tree_count(const TreeArgs a) {
    __shared__ int lds[4];
    int f[4];
    load_flags(a.work.top, (int64_t)blockIdx.x * kChunk + 4 * threadIdx.x, a.n, f);
    int total;
    block_scan(f[0] + f[1] + f[2] + f[3], lds, &total);
    if (threadIdx.x == 0) a.work.partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_tree_scan(const TreeArgs a) {
    __shared__ int lds[4];
    int carry = 0;
    for (int base = 0; base < a.work.chunks; base += kChunk) {
        const int i = base + 4 * (int)threadIdx.x;
        int f[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = i + k < a.work.chunks ? a.work.partial[i + k] : 0;
        int total;
        int at = carry + block_scan(f[0] + f[1] + f[2] + f[3], lds, &total);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i + k < a.work.chunks) a.work.partial[i + k] = at;
            at += f[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0) a.work.head[0] = (uint32_t)carry;
}

__global__ __launch_bounds__(256) void k_tree_number(const TreeArgs a) {
    __shared__ int lds[4];
    const int64_t i = (int64_t)blockIdx.x * kChunk + 4 * threadIdx.x;
    int f[4];
    load_flags(a.work.top, i, a.n, f);
    int total;
    int at = a.work.partial[blockIdx.x] + block_scan(f[0] + f[1] + f[2] + f[3], lds, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (f[k]) a.work.top[i + k] = ++at;
    }
}

// ---- 4
__global__ __launch_bounds__(256) void k_tree_jump(int32_t* root, int n, uint32_t* changed, int round) {
    if (round > 0 && changed[round - 1] == 0u) return;
    bool any = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int p = __hip_atomic_load(root + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p < 0 || p == i) continue;
        const int g = __hip_atomic_load(root + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g == p) continue;
        __hip_atomic_store(root + i, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        any = true;
    }
    if (__any(any) && (threadIdx.x & 63) == 0) __hip_atomic_store(changed + round, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 5
template <bool VEC>
__global__ __launch_bounds__(256) void k_tree_label(const TreeArgs a) {
    const int c = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (c >= a.w) return;
    const float none = nodata();
    for (int r = blockIdx.y; r < a.h; r += gridDim.y) {
        const int i0 = r * a.w + c;
        float vid[4] = {none, none, none, none}, vh[4] = {none, none, none, none};
        int rt[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) rt[j] = c + j < a.w ? a.work.root[i0 + j] : -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (rt[j] < 0) continue;
            const int id = a.work.top[rt[j]];
            if (id <= 0) continue;
            const int rr = rt[j] / a.w, rc = rt[j] - rr * a.w;
            const float hr = a.src[(int64_t)rr * a.stride + rc];
            const float hc = a.src[(int64_t)r * a.stride + c + j];
            if (!labelled(hc, r, c + j, hr, rr, rc, a.k)) continue;
            atomicAdd(a.work.count + rt[j], 1);
            if (id_exact(id)) { vid[j] = id_value(id); vh[j] = hr; }
        }
        float* di = a.id_dst + (int64_t)r * a.id_stride + c;
        float* dh = a.height_dst ? a.height_dst + (int64_t)r * a.height_stride + c : nullptr;
        if (VEC && c + 4 <= a.w) {
            __builtin_nontemporal_store(pcr_f4v{vid[0], vid[1], vid[2], vid[3]}, reinterpret_cast<pcr_f4v*>(di));
            if (dh) __builtin_nontemporal_store(pcr_f4v{vh[0], vh[1], vh[2], vh[3]}, reinterpret_cast<pcr_f4v*>(dh));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (c + j >= a.w) continue;
                di[j] = vid[j];
                if (dh) dh[j] = vh[j];
            }
        }
    }
}

// ---- 6
struct TableArgs {
    const float* src;
    int w, n;
    int64_t stride;
    const int32_t* top;
    const int32_t* count;
    int64_t rows_cap;
    int32_t* rows;
    int32_t* cols;
    float* heights;
    int32_t* crown_cells;
};

__global__ __launch_bounds__(256) void k_tree_table(const TableArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        const int id = a.top[i];
        if (id <= 0 || id > a.rows_cap) continue;
        const int r = (int)(i / a.w), c = (int)(i - (int64_t)r * a.w);
        if (a.rows) a.rows[id - 1] = r;
        if (a.cols) a.cols[id - 1] = c;
        if (a.heights) a.heights[id - 1] = a.src[(int64_t)r * a.stride + c];
        if (a.crown_cells) a.crown_cells[id - 1] = a.count[i];
    }
}

// ---- the argument checks every entry point shares
int check_params(const std::string& fn, const pcr_hip_tree_params* p, Consts* k) {
    PCR_REQUIRE(std::isfinite(p->min_height), fn + ": min_height must be finite");
    PCR_REQUIRE(std::isfinite(p->window_base) && p->window_base >= 0.0f, fn + ": window_base must be finite and not negative");
    PCR_REQUIRE(std::isfinite(p->window_slope) && p->window_slope >= 0.0f, fn + ": window_slope must be finite and not negative");
    PCR_REQUIRE(p->max_radius_cells >= 1 && p->max_radius_cells <= kMaxRadius, fn + ": max_radius_cells must be between 1 and 32");
    PCR_REQUIRE(std::isfinite(p->min_crown_height), fn + ": min_crown_height must be finite");
    PCR_REQUIRE(p->crown_ratio >= 0.0f && p->crown_ratio <= 1.0f, fn + ": crown_ratio must be between 0 and 1");
    PCR_REQUIRE(p->max_crown_radius > 0.0f, fn + ": max_crown_radius must be positive (+Inf: no limit)");
    PCR_REQUIRE(p->stop_after >= 0 && p->stop_after <= 4, fn + ": stop_after must be between 0 and 4");
    const double cell = std::max(std::fabs(p->cell_size_x), std::fabs(p->cell_size_y));
    const double kk = k_of(cell);
    PCR_REQUIRE(std::isfinite(kk), fn + ": 0.5 / cell is not finite (cell sizes must not both be zero, none may be NaN)");
    k->min_height = p->min_height;
    k->window_base = p->window_base;
    k->window_slope = p->window_slope;
    k->max_radius = p->max_radius_cells;
    k->min_crown_height = p->min_crown_height;
    k->crown_ratio = p->crown_ratio;
    k->k = kk;
    k->M = M_of(p->max_crown_radius, cell);
    return PCR_HIP_OK;
}
int check_cells(const std::string& fn, int width, int height) {
    PCR_REQUIRE((int64_t)width * height <= 2147483647LL, fn + ": more than 2^31 - 1 cells");
    return PCR_HIP_OK;
}
int check_work(const std::string& fn, const void* d_work, size_t work_bytes, int width, int height) {
    PCR_REQUIRE(work_bytes >= work_bytes_of(width, height), fn + ": work_bytes too small (pcr_hip_trees_work_bytes)");
    (void)d_work;
    return PCR_HIP_OK;
}

}  // namespace
}  // namespace pcrhip

using namespace pcrhip;

extern "C" int pcr_hip_trees_work_bytes(int width, int height, size_t* bytes) {
    if (int rc = band::check_extent("trees_work_bytes", bytes != nullptr, width, height)) return rc;
    if (int rc = check_cells("trees_work_bytes", width, height)) return rc;
    *bytes = work_bytes_of(width, height);
    return PCR_HIP_OK;
}

extern "C" int pcr_hip_trees(const float* src, int width, int height, int64_t src_stride, const pcr_hip_tree_params* params,
                             float* id_dst, int64_t id_stride, float* height_dst, int64_t height_stride, void* d_work,
                             size_t work_bytes, pcr_hip_stream s) {
    const std::string fn = "trees";
    if (int rc = band::check_extent(fn, src && params && id_dst && d_work, width, height)) return rc;
    if (int rc = band::check_stride(fn, "src", src_stride, width)) return rc;
    if (int rc = band::check_stride(fn, "id", id_stride, width)) return rc;
    if (height_dst)
        if (int rc = band::check_stride(fn, "height", height_stride, width)) return rc;
    TreeArgs a{};
    if (int rc = check_params(fn, params, &a.k)) return rc;
    if (int rc = check_cells(fn, width, height)) return rc;
    if (int rc = check_work(fn, d_work, work_bytes, width, height)) return rc;
    {
        const band::Span sb = band::span_of(src, width, height, src_stride), ib = band::span_of(id_dst, width, height, id_stride);
        const band::Span wb = band::span_of(d_work, work_bytes);
        PCR_REQUIRE(!band::overlap(sb, ib), "trees: id_dst overlaps src");
        PCR_REQUIRE(!band::overlap(sb, wb), "trees: the workspace overlaps src");
        PCR_REQUIRE(!band::overlap(ib, wb), "trees: the workspace overlaps id_dst");
        if (height_dst) {
            const band::Span hb = band::span_of(height_dst, width, height, height_stride);
            PCR_REQUIRE(!band::overlap(sb, hb), "trees: height_dst overlaps src");
            PCR_REQUIRE(!band::overlap(ib, hb), "trees: height_dst overlaps id_dst");
            PCR_REQUIRE(!band::overlap(hb, wb), "trees: the workspace overlaps height_dst");
        }
    }
    if (int rc = band::check_tile_rows(fn, height, kTileH)) return rc;

    a.src = src;
    a.w = width;
    a.h = height;
    a.stride = src_stride;
    a.n = width * height;
    a.work = carve(d_work, width, height);
    a.id_dst = id_dst;
    a.height_dst = height_dst;
    a.id_stride = id_stride;
    a.height_stride = height_stride;
    a.wvec = width % 4 == 0;
    a.dvec = band::aligned16(id_dst, id_stride) && (!height_dst || band::aligned16(height_dst, height_stride));
    hipStream_t st = static_cast<hipStream_t>(s);

    PCR_HIP_TRY(hipMemsetAsync(a.work.head, 0, kHeadWords * 4, st));
    const dim3 tiles((width + kTileW - 1) / kTileW, (height + kTileH - 1) / kTileH);
    if (band::aligned16(src, src_stride)) hipLaunchKernelGGL((k_tree_cells<true>), tiles, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_tree_cells<false>), tiles, dim3(256), 0, st, a);
    const int phases = params->stop_after ? params->stop_after : 5;
    if (phases >= 2) hipLaunchKernelGGL(k_tree_disc, dim3((unsigned)(((int64_t)a.n + 255) / 256)), dim3(256), 0, st, a);
    if (phases < 3) {
        PCR_HIP_TRY(hipGetLastError());
        return PCR_HIP_OK;
    }
    hipLaunchKernelGGL(k_tree_count, dim3(a.work.chunks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_tree_scan, dim3(1), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_tree_number, dim3(a.work.chunks), dim3(256), 0, st, a);
    int rounds = 1;
    while (((int64_t)1 << rounds) < (int64_t)a.n) ++rounds;                       // ceil(log2(n)), at least 1
    rounds = std::min(rounds + 1, kMaxRounds);
    const unsigned jump_blocks = (unsigned)std::min<int64_t>(((int64_t)a.n + 255) / 256, 8192);
    for (int k = 0; k < rounds && phases >= 4; ++k)
        hipLaunchKernelGGL(k_tree_jump, dim3(jump_blocks), dim3(256), 0, st, a.work.root, a.n, a.work.head + kChangedAt, k);
    const dim3 rows((width + 1023) / 1024, height < 65535 ? height : 65535);
    if (phases < 5) {
        PCR_HIP_TRY(hipGetLastError());
        return PCR_HIP_OK;
    }
    if (a.dvec) hipLaunchKernelGGL((k_tree_label<true>), rows, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_tree_label<false>), rows, dim3(256), 0, st, a);
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

extern "C" int pcr_hip_trees_count(const void* d_work, size_t work_bytes, int64_t* n, int* rounds_worked, pcr_hip_stream s) {
    PCR_REQUIRE(d_work && n, "trees_count: null argument");
    PCR_REQUIRE(work_bytes >= 16 + (size_t)kHeadWords * 4, "trees_count: work_bytes too small (pcr_hip_trees_work_bytes)");
    uint32_t head[kHeadWords];
    const void* base = reinterpret_cast<const void*>((reinterpret_cast<uintptr_t>(d_work) + 15) & ~(uintptr_t)15);
    hipStream_t st = static_cast<hipStream_t>(s);
    PCR_HIP_TRY(hipMemcpyAsync(head, base, sizeof(head), hipMemcpyDeviceToHost, st));
    PCR_HIP_TRY(hipStreamSynchronize(st));
    *n = (int64_t)head[0];
    if (rounds_worked) {
        *rounds_worked = 0;
        for (int k = kChangedAt; k < kHeadWords; ++k) *rounds_worked += head[k] ? 1 : 0;
    }
    return PCR_HIP_OK;
}

extern "C" int pcr_hip_trees_table(const float* src, int width, int height, int64_t src_stride, const void* d_work,
                                   size_t work_bytes, int64_t n, int32_t* d_rows, int32_t* d_cols, float* d_heights,
                                   int32_t* d_crown_cells, pcr_hip_stream s) {
    const std::string fn = "trees_table";
    if (int rc = band::check_extent(fn, src && d_work, width, height)) return rc;
    if (int rc = band::check_stride(fn, "src", src_stride, width)) return rc;
    if (int rc = check_cells(fn, width, height)) return rc;
    if (int rc = check_work(fn, d_work, work_bytes, width, height)) return rc;
    PCR_REQUIRE(n >= 0, "trees_table: n must not be negative");
    if (n == 0) return PCR_HIP_OK;
    const Work k = carve(const_cast<void*>(d_work), width, height);
    TableArgs a{};
    a.src = src;
    a.w = width;
    a.n = width * height;
    a.stride = src_stride;
    a.top = k.top;
    a.count = k.count;
    a.rows_cap = n;
    a.rows = d_rows;
    a.cols = d_cols;
    a.heights = d_heights;
    a.crown_cells = d_crown_cells;
    const unsigned blocks = (unsigned)std::min<int64_t>(((int64_t)a.n + 255) / 256, 8192);
    hipLaunchKernelGGL(k_tree_table, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(s), a);
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

extern "C" int pcr_hip_trees_host(const float* src, int width, int height, int64_t src_stride, const pcr_hip_tree_params* params,
                                  float* id_dst, int64_t id_stride, float* height_dst, int64_t height_stride, int64_t* n,
                                  int64_t capacity, int32_t* rows, int32_t* cols, float* heights, int32_t* crown_cells) {
    const std::string fn = "trees_host";
    if (int rc = band::check_extent(fn, src && params && id_dst, width, height)) return rc;
    if (int rc = band::check_stride(fn, "src", src_stride, width)) return rc;
    if (int rc = band::check_stride(fn, "id", id_stride, width)) return rc;
    if (height_dst)
        if (int rc = band::check_stride(fn, "height", height_stride, width)) return rc;
    Consts k;
    if (int rc = check_params(fn, params, &k)) return rc;
    if (int rc = check_cells(fn, width, height)) return rc;
    PCR_REQUIRE(capacity >= 0, "trees_host: capacity must not be negative");
    {
        const band::Span sb = band::span_of(src, width, height, src_stride), ib = band::span_of(id_dst, width, height, id_stride);
        PCR_REQUIRE(!band::overlap(sb, ib), "trees_host: id_dst overlaps src");
        if (height_dst) {
            const band::Span hb = band::span_of(height_dst, width, height, height_stride);
            PCR_REQUIRE(!band::overlap(sb, hb), "trees_host: height_dst overlaps src");
            PCR_REQUIRE(!band::overlap(ib, hb), "trees_host: height_dst overlaps id_dst");
        }
    }
    HostTable t;
    const int64_t T = host(src, width, height, src_stride, k, id_dst, id_stride, height_dst, height_stride, &t);
    if (n) *n = T;
    const size_t m = (size_t)std::min(T, capacity);
    if (rows) std::copy_n(t.row.begin(), m, rows);
    if (cols) std::copy_n(t.col.begin(), m, cols);
    if (heights) std::copy_n(t.height.begin(), m, heights);
    if (crown_cells) std::copy_n(t.crown_cells.begin(), m, crown_cells);
    return PCR_HIP_OK;
}
