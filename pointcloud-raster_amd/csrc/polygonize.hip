// polygonize.hip -- pcr_hip_polygonize_*: the zones of a label band as rings of lattice corners (the contract: polygonize.hpp;
// include/pcr_hip.h "polygonize"), and what goes with it: the work areas' sizes, the counts, the ring table,
// the host twin.
//
// Two work areas, both the caller's.  The CELL area (2 bytes a cell) holds a head of 128 words -- E, R, V and one "changed" word
// per doubling round -- one partial sum per 1024 cells and one uint16 code per cell: the cell's boundary sides in the low four
// bits, above them the number of boundary edges of the cells before it in its chunk.  So the compact index of edge (cell, s) is
// partial[cell / 1024] + (code >> 4) + popcount(code & ((1 << s) - 1)): compact order IS slot order, and anyone who knows a slot
// finds its edge with two loads, no hash, no search.  The RING area (29 bytes an edge), sized once E is known, holds per edge its
// slot, its successor, its ring's key, its corner flag and two 64-bit words A and B that the doubling rounds ping-pong between.
// The launches, all on the caller's stream, none waited for:
//   pcr_hip_polygonize_edges
//     1  k_pg_cells     a workgroup per 1024 cells, a lane per four: zone, sides (the four neighbours come from L2: the band is
//                       read from HBM once), the chunk's scan, the codes and the chunk's sum
//     2  k_pg_scan      one workgroup: the exclusive scan of the chunk sums; E stays in the head
//   pcr_hip_polygonize_rings
//     3  k_pg_edges     a lane per cell: per boundary side the slot, the successor's compact index (polygonize.hpp's rule on
//                       the 3 x 3 zones, then the neighbour cell's code), the corner flag, and A = (m, j) = (slot or none, next)
//     4  k_pg_key       ceil(log2 E) + 1 rounds of m[e] = min(m[e], m[j[e]]), j[e] = j[j[e]], reading one buffer and writing the
//                       other, so a round reads only what the launch before wrote: every round's result, and the number of
//                       rounds that change something, is the same in every run.  (m, j) of e covers the 2^k edges from e on;
//                       on a cycle the cover wraps, which a minimum does not mind.  A round that lowers no m leaves every m at
//                       its cycle's minimum (m does not decrease along e, j[e], j[j[e]], ..., whose covers pass the minimum),
//                       so the next rounds return at once.  The "changed" word is set by a relaxed atomic store of 1: every
//                       writer stores the same value.
//     5  k_pg_rank_init, k_pg_rank   each cycle cut in front of its key edge; (d, j) = (corner flag, next or none) doubled the
//                       same way: d[e] ends as the number of corner edges from e to the cut, so the ring has d[key edge]
//                       vertices and e's vertex is number d[key edge] - d[e]
//     6  k_pg_ring_count, k_pg_scan x 2   key edges and their vertices per 1024 edges, scanned: R and V stay in the head
//   pcr_hip_polygonize_fetch
//     7  k_pg_ring_emit the chunk's scan again: key edge number k (in slot order, so in key order) stores ring k's zone and
//                       first vertex, into the caller's arrays and, the first vertex, into the free one of A and B
//     8  k_pg_vertices  a lane per edge: a corner edge finds its key edge by slot and stores its lattice corner
// Which of A and B holds a phase's result follows from the "changed" words alone; the kernels work it out (rounds_run).
// No kernel uses LDS beyond a scan's four words, none uses scratch.  Measured: profiles/polygonize.md.
#include "band_pass.hpp"
#include "polygonize.hpp"

#include <algorithm>

namespace pcrhip {
namespace {

namespace pg = polygonize;
using u64 = unsigned long long;

constexpr int kChunk = 1024;                                     // cells, or edges, per partial sum
constexpr int kHeadWords = 128;
constexpr int kMaxRounds = 40;
constexpr int kEdgesAt = 0, kRingsAt = 1, kVerticesAt = 2, kKeyChangedAt = 8, kRankChangedAt = 48;
static_assert(kRankChangedAt + kMaxRounds <= kHeadWords, "the head holds both phases' words");

size_t pad4(int64_t n) { return (size_t)((n + 3) & ~(int64_t)3); }
int64_t chunks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }

struct Cells {
    uint32_t* head;
    uint32_t* partial;               // [chunks]: boundary edges of the chunks before (after k_pg_scan)
    uint16_t* code;                  // [cells]
    int64_t chunks;
};
size_t cells_bytes_of(int width, int height) {
    const int64_t n = (int64_t)width * height;
    return 16 + (size_t)kHeadWords * 4 + pad4(chunks_of(n)) * 4 + pad4((n + 1) / 2) * 4;
}
Cells carve_cells(const void* d_work, int width, int height) {
    const int64_t n = (int64_t)width * height;
    Cells k;
    k.head = reinterpret_cast<uint32_t*>((reinterpret_cast<uintptr_t>(d_work) + 15) & ~(uintptr_t)15);
    k.partial = k.head + kHeadWords;
    k.chunks = chunks_of(n);
    k.code = reinterpret_cast<uint16_t*>(k.partial + pad4(k.chunks));
    return k;
}

struct Rings {
    u64* a;                          // [E] each: (m, j), then (d, j), then the rings' first vertices
    u64* b;
    uint32_t* slot;
    uint32_t* succ;
    uint32_t* key;
    uint32_t* ring_count;            // [chunks of edges]: key edges, then the rings before
    uint32_t* ring_len;              //                    their vertices, then the vertices before
    uint8_t* corner;
    int64_t chunks;
};
size_t rings_bytes_of(int64_t E) {
    return 16 + 2 * pad4(E) * 8 + 3 * pad4(E) * 4 + 2 * pad4(chunks_of(E)) * 4 + pad4(E);
}
Rings carve_rings(const void* d_work, int64_t E) {
    Rings k;
    k.a = reinterpret_cast<u64*>((reinterpret_cast<uintptr_t>(d_work) + 15) & ~(uintptr_t)15);
    k.b = k.a + pad4(E);
    k.slot = reinterpret_cast<uint32_t*>(k.b + pad4(E));
    k.succ = k.slot + pad4(E);
    k.key = k.succ + pad4(E);
    k.chunks = chunks_of(E);
    k.ring_count = k.key + pad4(E);
    k.ring_len = k.ring_count + pad4(k.chunks);
    k.corner = reinterpret_cast<uint8_t*>(k.ring_len + pad4(k.chunks));
    return k;
}

struct Args {
    pg::Band band;
    int64_t n;                       // cells
    int64_t E;                       // boundary edges, as the caller was told
    Cells cells;
    Rings rings;
    int key_rounds, rank_rounds;     // as launched
};

__host__ __device__ __forceinline__ u64 pack(uint32_t hi, uint32_t lo) { return ((u64)hi << 32) | lo; }
__host__ __device__ __forceinline__ uint32_t hi_of(u64 x) { return (uint32_t)(x >> 32); }
__host__ __device__ __forceinline__ uint32_t lo_of(u64 x) { return (uint32_t)x; }

// v's exclusive prefix over the workgroup's 256 lanes; total: the sum of all
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(s, off);
        if (lane >= off) s += o;
    }
    __syncthreads();                                             // (lds may still be read from the call before)
    if (lane == 63) lds[wave] = s;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t x = lds[k];
        if (k < wave) before += x;
        all += x;
    }
    *total = all;
    return before + s - v;
}

// The rounds of a doubling phase that ran: round k returns at once when round k - 1 changed nothing.
__device__ __forceinline__ int rounds_run(const uint32_t* changed, int rounds) {
    int k = 0;
    while (k < rounds && (k == 0 || changed[k - 1] != 0u)) ++k;
    return k;
}
// The edges the ring kernels work on: the caller's n_edges, and never more than k_pg_scan counted -- what lies beyond was never
// written.
__device__ __forceinline__ int64_t edges_of(const Args& a) {
    const int64_t counted = (int64_t)a.cells.head[kEdgesAt];
    return a.E < counted ? a.E : counted;
}
// The compact index of the edge with this slot.
__device__ __forceinline__ uint32_t edge_of(const Cells& k, uint32_t slot) {
    const uint32_t cell = slot >> 2, code = k.code[cell];
    return k.partial[cell >> 10] + (code >> 4) + (uint32_t)__popc(code & ((1u << (slot & 3u)) - 1u));
}

// ---- 1
__global__ __launch_bounds__(256) void k_pg_cells(const Args a) {
    __shared__ uint32_t lds[4];
    const int64_t i0 = (int64_t)blockIdx.x * kChunk + 4 * threadIdx.x;
    unsigned m[4] = {0, 0, 0, 0};
    if (i0 < a.n) {
        int r = (int)(i0 / a.band.w), c = (int)(i0 - (int64_t)r * a.band.w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < a.n) {
                const uint32_t z = a.band.zone(r, c);
                if (z != 0u) m[k] = pg::sides_of(a.band, r, c, z);
            }
            if (++c == a.band.w) { c = 0; ++r; }
        }
    }
    uint32_t total;
    uint32_t at = block_scan((uint32_t)(__popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3])), lds, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i0 + k < a.n) a.cells.code[i0 + k] = (uint16_t)((at << 4) | m[k]);
        at += (uint32_t)__popc(m[k]);
    }
    if (threadIdx.x == 0) a.cells.partial[blockIdx.x] = total;
}

// ---- 2: p[0 .. count) into its exclusive scan, the sum into *total
__global__ __launch_bounds__(256) void k_pg_scan(uint32_t* p, int64_t count, uint32_t* total) {
    __shared__ uint32_t lds[4];
    uint32_t carry = 0;
    for (int64_t base = 0; base < count; base += kChunk) {
        const int64_t i = base + 4 * (int64_t)threadIdx.x;
        uint32_t f[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = i + k < count ? p[i + k] : 0u;
        uint32_t all;
        uint32_t at = carry + block_scan(f[0] + f[1] + f[2] + f[3], lds, &all);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i + k < count) p[i + k] = at;
            at += f[k];
        }
        carry += all;
    }
    if (threadIdx.x == 0) *total = carry;
}

// ---- 3
__global__ __launch_bounds__(256) void k_pg_edges(const Args a) {
    const uint32_t E = (uint32_t)edges_of(a);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        const uint32_t code = a.cells.code[i];
        const unsigned m = code & 15u;
        if (m == 0u) continue;
        const int r = (int)(i / a.band.w), c = (int)(i - (int64_t)r * a.band.w);
        const uint32_t z = a.band.zone(r, c);
        uint32_t e = a.cells.partial[i >> 10] + (code >> 4);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (!((m >> s) & 1u)) continue;
            if (e < E) {                                             // (an n_edges below the count: nothing is stored past it)
                int nr, nc, ns;
                pg::successor(a.band, r, c, s, z, nr, nc, ns);
                uint32_t next = edge_of(a.cells, 4u * (uint32_t)((int64_t)nr * a.band.w + nc) + (uint32_t)ns);
                if (next >= E) next = e;
                const uint32_t slot = 4u * (uint32_t)i + (uint32_t)s;
                const bool corner = pg::is_corner(a.band, r, c, s, z);
                a.rings.slot[e] = slot;
                a.rings.succ[e] = next;
                a.rings.corner[e] = corner ? 1 : 0;
                a.rings.a[e] = pack(corner ? slot : pg::kNone, next);
            }
            ++e;
        }
    }
}

// A round's "changed" word: a relaxed agent-scope store of 1, by the first waves only -- the load ahead of it is served by L2, and
// a hundred thousand waves storing to one address cost a round more than its edges did (profiles/polygonize.md).
__device__ __forceinline__ void set_changed(uint32_t* word) {
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
        __hip_atomic_store(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 4
__global__ __launch_bounds__(256) void k_pg_key(const Args a, int round) {
    uint32_t* changed = a.cells.head + kKeyChangedAt;
    if (round > 0 && changed[round - 1] == 0u) return;
    const u64* in = round & 1 ? a.rings.b : a.rings.a;
    u64* out = round & 1 ? a.rings.a : a.rings.b;
    bool any = false;
    const int64_t E = edges_of(a);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
        const u64 mine = in[e], there = in[lo_of(mine)];
        const uint32_t m = min(hi_of(mine), hi_of(there));
        out[e] = pack(m, lo_of(there));
        any = any || m != hi_of(mine);
    }
    if (__any(any) && (threadIdx.x & 63) == 0) set_changed(changed + round);
}

// ---- 5
__global__ __launch_bounds__(256) void k_pg_rank_init(const Args a) {
    const u64* keys = rounds_run(a.cells.head + kKeyChangedAt, a.key_rounds) & 1 ? a.rings.b : a.rings.a;
    const int64_t E = edges_of(a);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
        const uint32_t key = hi_of(keys[e]);                         // (read before a[e] is stored: `keys` may be a)
        const uint32_t next = a.rings.succ[e];
        a.rings.key[e] = key;
        a.rings.a[e] = pack(a.rings.corner[e], a.rings.slot[next] == key ? pg::kNone : next);
    }
}
__global__ __launch_bounds__(256) void k_pg_rank(const Args a, int round) {
    uint32_t* changed = a.cells.head + kRankChangedAt;
    if (round > 0 && changed[round - 1] == 0u) return;
    const u64* in = round & 1 ? a.rings.b : a.rings.a;
    u64* out = round & 1 ? a.rings.a : a.rings.b;
    bool any = false;
    const int64_t E = edges_of(a);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
        u64 mine = in[e];
        if (lo_of(mine) != pg::kNone) {
            const u64 there = in[lo_of(mine)];
            mine = pack(hi_of(mine) + hi_of(there), lo_of(there));
            any = true;
        }
        out[e] = mine;
    }
    if (__any(any) && (threadIdx.x & 63) == 0) set_changed(changed + round);
}

// ---- 6, 7: the key edges of a chunk of 1024 edges and their rings' lengths
__device__ __forceinline__ const u64* ranks_of(const Args& a) {
    return rounds_run(a.cells.head + kRankChangedAt, a.rank_rounds) & 1 ? a.rings.b : a.rings.a;
}
__device__ __forceinline__ void load_keys(const Args& a, const u64* ranks, int64_t e0, uint32_t is_key[4], uint32_t len[4]) {
    const int64_t E = edges_of(a);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t e = e0 + k;
        is_key[k] = e < E && a.rings.corner[e] && a.rings.key[e] == a.rings.slot[e] ? 1u : 0u;
        len[k] = is_key[k] ? hi_of(ranks[e]) : 0u;
    }
}
__global__ __launch_bounds__(256) void k_pg_ring_count(const Args a) {
    __shared__ uint32_t lds[4];
    uint32_t is_key[4], len[4], rings, vertices;
    load_keys(a, ranks_of(a), (int64_t)blockIdx.x * kChunk + 4 * threadIdx.x, is_key, len);
    block_scan(is_key[0] + is_key[1] + is_key[2] + is_key[3], lds, &rings);
    block_scan(len[0] + len[1] + len[2] + len[3], lds, &vertices);
    if (threadIdx.x == 0) {
        a.rings.ring_count[blockIdx.x] = rings;
        a.rings.ring_len[blockIdx.x] = vertices;
    }
}

struct FetchArgs {
    Args a;
    int64_t R, V;
    uint32_t* ring_zone;
    int64_t* ring_offset;
    int32_t* vertex_row;
    int32_t* vertex_col;
};
__global__ __launch_bounds__(256) void k_pg_ring_emit(const FetchArgs f) {
    __shared__ uint32_t lds[4];
    const Args& a = f.a;
    const u64* ranks = ranks_of(a);
    u64* first = ranks == a.rings.a ? a.rings.b : a.rings.a;
    const int64_t e0 = (int64_t)blockIdx.x * kChunk + 4 * threadIdx.x;
    uint32_t is_key[4], len[4], all;
    load_keys(a, ranks, e0, is_key, len);
    uint32_t ring = a.rings.ring_count[blockIdx.x] + block_scan(is_key[0] + is_key[1] + is_key[2] + is_key[3], lds, &all);
    uint32_t at = a.rings.ring_len[blockIdx.x] + block_scan(len[0] + len[1] + len[2] + len[3], lds, &all);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!is_key[k]) continue;
        first[e0 + k] = (u64)at;
        if ((int64_t)ring < f.R) {
            const uint32_t cell = a.rings.slot[e0 + k] >> 2;
            const int r = (int)(cell / (uint32_t)a.band.w), c = (int)(cell - (uint32_t)r * (uint32_t)a.band.w);
            f.ring_zone[ring] = a.band.zone(r, c);
            f.ring_offset[ring] = (int64_t)at;
        }
        ++ring;
        at += len[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) f.ring_offset[f.R] = f.V;
}

// ---- 8
__global__ __launch_bounds__(256) void k_pg_vertices(const FetchArgs f) {
    const Args& a = f.a;
    const u64* ranks = ranks_of(a);
    const u64* first = ranks == a.rings.a ? a.rings.b : a.rings.a;
    const int64_t E = edges_of(a);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
        if (!a.rings.corner[e]) continue;
        const uint32_t k = edge_of(a.cells, a.rings.key[e]);
        if ((int64_t)k >= E) continue;
        const int64_t v = (int64_t)first[k] + (int64_t)(hi_of(ranks[k]) - hi_of(ranks[e]));
        if (v < 0 || v >= f.V) continue;
        const uint32_t slot = a.rings.slot[e], cell = slot >> 2;
        const int r = (int)(cell / (uint32_t)a.band.w), c = (int)(cell - (uint32_t)r * (uint32_t)a.band.w);
        f.vertex_row[v] = pg::corner_row(r, (int)(slot & 3u));
        f.vertex_col[v] = pg::corner_col(c, (int)(slot & 3u));
    }
}

// ---- the checks the entry points share: the same messages on the device path and on the host twin's
int check_band(const std::string& fn, bool pointers, int width, int height, int64_t stride) {
    if (int rc = band::check_extent(fn, pointers, width, height)) return rc;
    PCR_REQUIRE(stride >= width, fn + ": stride smaller than width");
    PCR_REQUIRE((int64_t)width * height <= pg::kMaxCells, fn + ": more than 2^30 - 1 cells");
    return PCR_HIP_OK;
}
int check_cells_work(const std::string& fn, const float* d_band, int width, int height, int64_t stride, const void* d_work, size_t bytes) {
    PCR_REQUIRE(bytes >= cells_bytes_of(width, height), fn + ": cells_work_bytes too small (pcr_hip_polygonize_cells_work_bytes)");
    PCR_REQUIRE(!band::overlap(band::span_of(d_band, width, height, stride), band::span_of(d_work, bytes)),
                fn + ": the cell work area overlaps the band");
    return PCR_HIP_OK;
}
int check_rings_work(const std::string& fn, const float* d_band, int width, int height, int64_t stride, const void* d_cells,
                     size_t cells_bytes, int64_t E, const void* d_rings, size_t rings_bytes) {
    PCR_REQUIRE(E >= 1 && E <= 4 * (int64_t)width * height, fn + ": n_edges must be between 1 and 4 per cell");
    PCR_REQUIRE(rings_bytes >= rings_bytes_of(E), fn + ": rings_work_bytes too small (pcr_hip_polygonize_rings_work_bytes)");
    const band::Span rb = band::span_of(d_rings, rings_bytes);
    PCR_REQUIRE(!band::overlap(band::span_of(d_band, width, height, stride), rb), fn + ": the ring work area overlaps the band");
    PCR_REQUIRE(!band::overlap(band::span_of(d_cells, cells_bytes), rb), fn + ": the work areas overlap");
    return PCR_HIP_OK;
}
int rounds_for(int64_t E) {
    int r = 0;
    while (((int64_t)1 << r) < E) ++r;                             // ceil(log2 E)
    return std::min(r + 1, kMaxRounds);
}
unsigned stride_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 16384); }

Args args_of(const float* d_band, int width, int height, int64_t stride, const void* d_cells, int64_t E, const void* d_rings) {
    Args a{};
    a.band = pg::Band{d_band, width, height, stride};
    a.n = (int64_t)width * height;
    a.E = E;
    a.cells = carve_cells(d_cells, width, height);
    if (d_rings) a.rings = carve_rings(d_rings, E);
    a.key_rounds = a.rank_rounds = E > 0 ? rounds_for(E) : 0;
    return a;
}

}  // namespace
}  // namespace pcrhip

using namespace pcrhip;

extern "C" int pcr_hip_polygonize_cells_work_bytes(int width, int height, size_t* bytes) {
    if (int rc = check_band("polygonize_cells_work_bytes", bytes != nullptr, width, height, width)) return rc;
    *bytes = cells_bytes_of(width, height);
    return PCR_HIP_OK;
}

extern "C" int pcr_hip_polygonize_rings_work_bytes(int64_t n_edges, size_t* bytes) {
    PCR_REQUIRE(bytes, "polygonize_rings_work_bytes: null argument");
    PCR_REQUIRE(n_edges >= 0 && n_edges <= 4 * pg::kMaxCells, "polygonize_rings_work_bytes: n_edges must be between 0 and 2^32 - 4");
    *bytes = rings_bytes_of(n_edges);
    return PCR_HIP_OK;
}

extern "C" int pcr_hip_polygonize_edges(const float* d_band, int width, int height, int64_t stride, void* d_cells_work,
                                        size_t cells_work_bytes, pcr_hip_stream s) {
    const std::string fn = "polygonize";
    if (int rc = check_band(fn, d_band && d_cells_work, width, height, stride)) return rc;
    if (int rc = check_cells_work(fn, d_band, width, height, stride, d_cells_work, cells_work_bytes)) return rc;
    const Args a = args_of(d_band, width, height, stride, d_cells_work, 0, nullptr);
    hipStream_t st = static_cast<hipStream_t>(s);
    PCR_HIP_TRY(hipMemsetAsync(a.cells.head, 0, kHeadWords * 4, st));
    hipLaunchKernelGGL(k_pg_cells, dim3((unsigned)a.cells.chunks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_pg_scan, dim3(1), dim3(256), 0, st, a.cells.partial, a.cells.chunks, a.cells.head + kEdgesAt);
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

extern "C" int pcr_hip_polygonize_count(const void* d_cells_work, size_t cells_work_bytes, int64_t* n_edges, int64_t* n_rings,
                                        int64_t* n_vertices, int* key_rounds_worked, int* rank_rounds_worked, pcr_hip_stream s) {
    PCR_REQUIRE(d_cells_work && n_edges, "polygonize_count: null argument");
    PCR_REQUIRE(cells_work_bytes >= 16 + (size_t)kHeadWords * 4, "polygonize_count: cells_work_bytes too small (pcr_hip_polygonize_cells_work_bytes)");
    uint32_t head[kHeadWords];
    const void* base = reinterpret_cast<const void*>((reinterpret_cast<uintptr_t>(d_cells_work) + 15) & ~(uintptr_t)15);
    hipStream_t st = static_cast<hipStream_t>(s);
    PCR_HIP_TRY(hipMemcpyAsync(head, base, sizeof(head), hipMemcpyDeviceToHost, st));
    PCR_HIP_TRY(hipStreamSynchronize(st));
    *n_edges = (int64_t)head[kEdgesAt];
    if (n_rings) *n_rings = (int64_t)head[kRingsAt];
    if (n_vertices) *n_vertices = (int64_t)head[kVerticesAt];
    for (int phase = 0; phase < 2; ++phase) {
        int* out = phase ? rank_rounds_worked : key_rounds_worked;
        if (!out) continue;
        *out = 0;
        for (int k = 0; k < kMaxRounds; ++k) *out += head[(phase ? kRankChangedAt : kKeyChangedAt) + k] ? 1 : 0;
    }
    return PCR_HIP_OK;
}

extern "C" int pcr_hip_polygonize_rings(const float* d_band, int width, int height, int64_t stride, const void* d_cells_work,
                                        size_t cells_work_bytes, int64_t n_edges, void* d_rings_work, size_t rings_work_bytes,
                                        const pcr_hip_polygonize_params* params, pcr_hip_stream s) {
    const std::string fn = "polygonize";
    if (int rc = check_band(fn, d_band && d_cells_work && d_rings_work, width, height, stride)) return rc;
    if (int rc = check_cells_work(fn, d_band, width, height, stride, d_cells_work, cells_work_bytes)) return rc;
    if (int rc = check_rings_work(fn, d_band, width, height, stride, d_cells_work, cells_work_bytes, n_edges, d_rings_work, rings_work_bytes))
        return rc;
    const Args a = args_of(d_band, width, height, stride, d_cells_work, n_edges, d_rings_work);
    hipStream_t st = static_cast<hipStream_t>(s);
    auto mark = [&](int i) {
        return params && params->events[i] ? hipEventRecord(static_cast<hipEvent_t>(params->events[i]), st) : hipSuccess;
    };
    // (the head's words of this phase, so that the call may be repeated on one pcr_hip_polygonize_edges)
    PCR_HIP_TRY(hipMemsetAsync(a.cells.head + kRingsAt, 0, (kHeadWords - kRingsAt) * 4, st));
    hipLaunchKernelGGL(k_pg_edges, dim3(stride_blocks(a.n)), dim3(256), 0, st, a);
    PCR_HIP_TRY(mark(0));
    const unsigned blocks = stride_blocks(a.E);
    for (int k = 0; k < a.key_rounds; ++k) hipLaunchKernelGGL(k_pg_key, dim3(blocks), dim3(256), 0, st, a, k);
    PCR_HIP_TRY(mark(1));
    hipLaunchKernelGGL(k_pg_rank_init, dim3(blocks), dim3(256), 0, st, a);
    for (int k = 0; k < a.rank_rounds; ++k) hipLaunchKernelGGL(k_pg_rank, dim3(blocks), dim3(256), 0, st, a, k);
    PCR_HIP_TRY(mark(2));
    hipLaunchKernelGGL(k_pg_ring_count, dim3((unsigned)a.rings.chunks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_pg_scan, dim3(1), dim3(256), 0, st, a.rings.ring_count, a.rings.chunks, a.cells.head + kRingsAt);
    hipLaunchKernelGGL(k_pg_scan, dim3(1), dim3(256), 0, st, a.rings.ring_len, a.rings.chunks, a.cells.head + kVerticesAt);
    PCR_HIP_TRY(mark(3));
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

extern "C" int pcr_hip_polygonize_fetch(const float* d_band, int width, int height, int64_t stride, const void* d_cells_work,
                                        size_t cells_work_bytes, int64_t n_edges, void* d_rings_work, size_t rings_work_bytes,
                                        int64_t n_rings, int64_t n_vertices, uint32_t* d_ring_zone, int64_t* d_ring_offset,
                                        int32_t* d_vertex_row, int32_t* d_vertex_col, pcr_hip_stream s) {
    const std::string fn = "polygonize";
    if (int rc = check_band(fn, d_band && d_cells_work && d_rings_work && d_ring_zone && d_ring_offset && d_vertex_row && d_vertex_col,
                            width, height, stride))
        return rc;
    if (int rc = check_cells_work(fn, d_band, width, height, stride, d_cells_work, cells_work_bytes)) return rc;
    if (int rc = check_rings_work(fn, d_band, width, height, stride, d_cells_work, cells_work_bytes, n_edges, d_rings_work, rings_work_bytes))
        return rc;
    PCR_REQUIRE(n_rings >= 1 && n_rings <= n_edges && n_vertices >= 1 && n_vertices <= n_edges,
                fn + ": n_rings and n_vertices must be between 1 and n_edges");
    {
        const band::Span out[4] = {band::span_of(d_ring_zone, (size_t)n_rings * 4), band::span_of(d_ring_offset, ((size_t)n_rings + 1) * 8),
                                   band::span_of(d_vertex_row, (size_t)n_vertices * 4), band::span_of(d_vertex_col, (size_t)n_vertices * 4)};
        const band::Span in[3] = {band::span_of(d_band, width, height, stride), band::span_of(d_cells_work, cells_work_bytes),
                                  band::span_of(d_rings_work, rings_work_bytes)};
        bool clash = false;
        for (int i = 0; i < 4; ++i) {
            for (int j = 0; j < 3; ++j) clash = clash || band::overlap(out[i], in[j]);
            for (int j = 0; j < i; ++j) clash = clash || band::overlap(out[i], out[j]);
        }
        PCR_REQUIRE(!clash, fn + ": an output overlaps an input, a work area or another output");
    }
    FetchArgs f{};
    f.a = args_of(d_band, width, height, stride, d_cells_work, n_edges, d_rings_work);
    f.R = n_rings;
    f.V = n_vertices;
    f.ring_zone = d_ring_zone;
    f.ring_offset = d_ring_offset;
    f.vertex_row = d_vertex_row;
    f.vertex_col = d_vertex_col;
    hipStream_t st = static_cast<hipStream_t>(s);
    hipLaunchKernelGGL(k_pg_ring_emit, dim3((unsigned)f.a.rings.chunks), dim3(256), 0, st, f);
    hipLaunchKernelGGL(k_pg_vertices, dim3(stride_blocks(n_edges)), dim3(256), 0, st, f);
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

extern "C" int pcr_hip_polygonize_host(const float* band_data, int width, int height, int64_t stride, int64_t* n_edges, int64_t* n_rings,
                                       int64_t* n_vertices, int64_t ring_capacity, int64_t vertex_capacity, uint32_t* ring_zone,
                                       int64_t* ring_offset, int32_t* vertex_row, int32_t* vertex_col) {
    const std::string fn = "polygonize";
    if (int rc = check_band(fn, band_data != nullptr, width, height, stride)) return rc;
    PCR_REQUIRE(ring_capacity >= 0 && vertex_capacity >= 0, fn + ": a capacity must not be negative");
    pg::HostRings t;
    pg::host(pg::Band{band_data, width, height, stride}, &t);
    const int64_t R = (int64_t)t.ring_zone.size(), V = (int64_t)t.vertex_row.size();
    if (n_edges) *n_edges = t.edges;
    if (n_rings) *n_rings = R;
    if (n_vertices) *n_vertices = V;
    // the table, when all of it fits: a part of one would be of no use
    if (R <= ring_capacity && V <= vertex_capacity) {
        if (ring_zone) std::copy(t.ring_zone.begin(), t.ring_zone.end(), ring_zone);
        if (ring_offset) std::copy(t.ring_offset.begin(), t.ring_offset.end(), ring_offset);
        if (vertex_row) std::copy(t.vertex_row.begin(), t.vertex_row.end(), vertex_row);
        if (vertex_col) std::copy(t.vertex_col.begin(), t.vertex_col.end(), vertex_col);
    }
    return PCR_HIP_OK;
}
