// filter_classes.hip -- the pipelines' filter stage (PipelineConfig::filter as class 0, ReductionSpec::filter as the classes
// behind it): pcr_hip_filter_classes, pcr_hip_engine_touch.
//
//   k_filter_classes   ONE sweep over the points evaluates a table of DISTINCT predicates and stores one byte mask per filter
//                      CLASS (a class = the set of predicates it ANDs), in the layout pcr_hip_engine_set_point_mask takes.  A
//                      channel is loaded once per point however many predicates and classes read it, a predicate is evaluated
//                      once however many classes AND it.  Traffic per point: 4 B per distinct channel in, 1 B per class out --
//                      one pcr_hip_filter_mask call per class would read every channel of every class again.
//   k_touch            the touched-tile flags of the points the engine's current mask keeps, exactly as a Point scatter sets
//                      them (bounds, owned rows, the one-tile case, division as in world_to_cell), and nothing else: no plane is
//                      written.  A kernel of its own, not part of the sweep: the sweep never reads x, y, and the flags are only
//                      needed from here when no group of an ingest is unfiltered (else that group's scatter sets them).
//
// The predicates travel as kernel ARGUMENTS (wave-uniform, read through the scalar cache): 32 predicates x 80 B + 32 channel
// pointers + the class words = 2.9 KB of the 4 KB a kernel may take.  A table beyond 32 predicates would have to live in
// device memory; the pipeline refuses such a configuration instead.
#include "engine.hpp"

using namespace pcrhip;

namespace {

constexpr int kSweepThreads = 256;
constexpr int kTouchThreads = 256;

// Predicates sorted by channel: those of channel c are [first[c], first[c + 1]).  Bit k of cls[j]: class j ANDs predicate k.
struct ClassSweep {
    int n_ch, n_pred, n_cls;
    unsigned cls[PCR_HIP_MAX_FILTER_CLASSES];
    unsigned char first[PCR_HIP_MAX_CLASS_PREDICATES + 1];
    const float* ch[PCR_HIP_MAX_CLASS_PREDICATES];
    pcr_hip_predicate p[PCR_HIP_MAX_CLASS_PREDICATES];
};
static_assert(sizeof(ClassSweep) + 64 <= 4096, "the sweep's table must fit the kernel arguments");

// Bit k of fail[j]: point j of the lane's four fails predicate k.
__device__ __forceinline__ void eval_channel(const ClassSweep& t, int c, const float (&v)[4], unsigned (&fail)[4]) {
    for (int k = t.first[c]; k < t.first[c + 1]; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (!eval_pred(t.p[k], v[j])) fail[j] |= 1u << k;
    }
}

// NCH > 0: that many distinct channels, their loads issued together ahead of any compare; 0: any number, one after another.
// Every lane of a wave runs the same number of iterations (ballots inside): `groups` of four points in the vector part
// (16-byte channel loads, one packed 32-bit store per class: 256 contiguous bytes per wave), then the points behind the
// last whole group -- all of them when an array is not aligned for that -- one per lane.
template <int NCH>
__global__ void __launch_bounds__(kSweepThreads)
k_filter_classes(ClassSweep t, uint64_t n, uint64_t groups, unsigned char* __restrict__ masks, uint64_t stride,
                 unsigned long long* __restrict__ counts) {
    __shared__ unsigned lds_cnt[PCR_HIP_MAX_FILTER_CLASSES];
    if (threadIdx.x < PCR_HIP_MAX_FILTER_CLASSES) lds_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * kSweepThreads;
    const uint64_t tid = (uint64_t)blockIdx.x * kSweepThreads + threadIdx.x;
    const bool lane0 = (threadIdx.x & 63) == 0;
    const int n_ch = NCH > 0 ? NCH : t.n_ch;

    const uint64_t groups_round = ((groups + 63) / 64) * 64;
    for (uint64_t g = tid; g < groups_round; g += step) {
        const bool live = g < groups;
        unsigned fail[4] = {0u, 0u, 0u, 0u};
        if (live) {
            if (NCH > 0) {
                float4 v4[NCH > 0 ? NCH : 1];
#pragma unroll
                for (int c = 0; c < NCH; ++c) v4[c] = reinterpret_cast<const float4*>(t.ch[c])[g];
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const float v[4] = {v4[c].x, v4[c].y, v4[c].z, v4[c].w};
                    eval_channel(t, c, v, fail);
                }
            } else {
                for (int c = 0; c < n_ch; ++c) {
                    const float4 q = reinterpret_cast<const float4*>(t.ch[c])[g];
                    const float v[4] = {q.x, q.y, q.z, q.w};
                    eval_channel(t, c, v, fail);
                }
            }
        }
        for (int j = 0; j < t.n_cls; ++j) {
            const unsigned m = t.cls[j];
            const bool k0 = live && !(fail[0] & m), k1 = live && !(fail[1] & m), k2 = live && !(fail[2] & m),
                       k3 = live && !(fail[3] & m);
            if (live)
                reinterpret_cast<unsigned*>(masks + (uint64_t)j * stride)[g] =
                    (k0 ? 1u : 0u) | (k1 ? 0x100u : 0u) | (k2 ? 0x10000u : 0u) | (k3 ? 0x1000000u : 0u);
            if (counts) {                                   // (wave-uniform)
                const unsigned c = (unsigned)(__popcll(__ballot(k0)) + __popcll(__ballot(k1)) + __popcll(__ballot(k2)) +
                                              __popcll(__ballot(k3)));
                if (lane0 && c) atomicAdd(&lds_cnt[j], c);
            }
        }
    }

    const uint64_t first_pt = groups * 4;
    const uint64_t rest_round = ((n - first_pt + 63) / 64) * 64;
    for (uint64_t r = tid; r < rest_round; r += step) {
        const uint64_t i = first_pt + r;
        const bool live = i < n;
        unsigned fail = 0u;
        if (live)
            for (int c = 0; c < n_ch; ++c) {
                const float v = t.ch[c][i];
                for (int k = t.first[c]; k < t.first[c + 1]; ++k)
                    if (!eval_pred(t.p[k], v)) fail |= 1u << k;
            }
        for (int j = 0; j < t.n_cls; ++j) {
            const bool keep = live && !(fail & t.cls[j]);
            if (live) masks[(uint64_t)j * stride + i] = keep ? 1 : 0;
            if (counts) {
                const unsigned c = (unsigned)__popcll(__ballot(keep));
                if (lane0 && c) atomicAdd(&lds_cnt[j], c);
            }
        }
    }

    // one global atomic per (workgroup, class): a workgroup counts fewer than 2^32 points (n < 2^40, checked by the caller)
    if (counts) {
        __syncthreads();
        if ((int)threadIdx.x < t.n_cls && lds_cnt[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)lds_cnt[threadIdx.x]);
    }
}

// The flag bookkeeping of the counting passes (k_bin_count: TouchLds gathers a workgroup's tiles in LDS and flags them in
// memory once; one tile: the workgroup's first thread flags it), the validity test of every scatter kernel.
__global__ void __launch_bounds__(kTouchThreads)
k_touch(GridDev g_uniform, const double* __restrict__ x, const double* __restrict__ y, uint64_t n, uint32_t* __restrict__ touched) {
    const GridDev g = vector_resident<PCR_VRES_POINT>(g_uniform);
    __shared__ unsigned any_valid;
    __shared__ unsigned lds_touch[kTouchLdsTiles];
    TouchLds tl;
    tl.begin(g, lds_touch, kTouchThreads);
    if (threadIdx.x == 0) any_valid = 0u;
    __syncthreads();
    const bool one_tile = g.tiles_x * g.tiles_y == 1;
    bool mine = false;
    auto handle = [&](uint64_t i, double wx, double wy) {
        int col = 0, row = 0;
        bool valid = point_kept(g, i) && world_to_cell(g, wx, wy, col, row);
        valid = valid && row >= g.own_r0 && row < g.own_r1;
        if (!valid) return;
        mine = true;
        if (!one_tile) tl.touch(g, touched, row, col);
    };
    const uint64_t step = (uint64_t)gridDim.x * kTouchThreads;
    const uint64_t tid = (uint64_t)blockIdx.x * kTouchThreads + threadIdx.x;
    const bool aligned = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
    const uint64_t pairs = aligned ? n / 2 : 0;
    for (uint64_t p = tid; p < pairs; p += step) {                  // 16-byte loads, two points per lane
        const double2 xs = stream_load(reinterpret_cast<const double2*>(x) + p);
        const double2 ys = stream_load(reinterpret_cast<const double2*>(y) + p);
        handle(2 * p, xs.x, ys.x);
        handle(2 * p + 1, xs.y, ys.y);
    }
    for (uint64_t i = 2 * pairs + tid; i < n; i += step) handle(i, x[i], y[i]);
    if (mine) any_valid = 1u;                                       // (every writer stores 1)
    __syncthreads();
    tl.flush(g, touched, kTouchThreads);
    if (threadIdx.x == 0 && any_valid && one_tile) touched[0] = 1u;
}

unsigned blocks_for(uint64_t items, int threads) {
    const uint64_t b = (items + threads - 1) / threads;
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(b, 1), 2048);     // 8 workgroups per CU, grid-stride beyond
}

}  // namespace

extern "C" {

int pcr_hip_filter_classes(const pcr_hip_predicate* preds, int n_pred, const uint32_t* class_predicates, int n_classes, uint64_t n,
                           uint8_t* d_masks, uint64_t mask_stride, unsigned long long* d_counts, pcr_hip_stream s) {
    PCR_REQUIRE(n_classes >= 1 && n_classes <= PCR_HIP_MAX_FILTER_CLASSES, "filter_classes: 1..8 classes expected");
    PCR_REQUIRE(n_pred >= 0 && n_pred <= PCR_HIP_MAX_CLASS_PREDICATES, "filter_classes: more than 32 distinct predicates");
    PCR_REQUIRE(class_predicates, "filter_classes: null class table");
    PCR_REQUIRE(n_pred == 0 || preds, "filter_classes: null predicate table");
    PCR_REQUIRE(n < ((uint64_t)1 << 40), "filter_classes: too many points in one call");
    ClassSweep t{};
    t.n_pred = n_pred;
    t.n_cls = n_classes;
    const uint32_t known = n_pred == 32 ? 0xFFFFFFFFu : ((1u << n_pred) - 1u);
    for (int j = 0; j < n_classes; ++j)
        PCR_REQUIRE((class_predicates[j] & ~known) == 0, "filter_classes: a class names a predicate outside the table");
    // predicates grouped by channel, in order of first appearance; the class words follow the permutation
    int place[PCR_HIP_MAX_CLASS_PREDICATES];
    int at = 0;
    for (int k = 0; k < n_pred; ++k) {
        PCR_REQUIRE(preds[k].d_channel, "filter_points: null channel pointer");
        PCR_REQUIRE(preds[k].op >= 0 && preds[k].op <= PCR_HIP_CMP_NOT_IN_SET, "filter_points: unknown compare op");
        PCR_REQUIRE(preds[k].set_size >= 0 && preds[k].set_size <= PCR_HIP_MAX_FILTER_SET,
                    "filter_points: value_set larger than 16 entries");
        bool seen = false;
        for (int c = 0; c < t.n_ch; ++c) seen = seen || t.ch[c] == preds[k].d_channel;
        if (!seen) t.ch[t.n_ch++] = preds[k].d_channel;
    }
    for (int c = 0; c < t.n_ch; ++c) {
        t.first[c] = (unsigned char)at;
        for (int k = 0; k < n_pred; ++k)
            if (preds[k].d_channel == t.ch[c]) { place[k] = at; t.p[at++] = preds[k]; }
    }
    t.first[t.n_ch] = (unsigned char)at;
    for (int j = 0; j < n_classes; ++j)
        for (int k = 0; k < n_pred; ++k)
            if (class_predicates[j] >> k & 1u) t.cls[j] |= 1u << place[k];
    hipStream_t st = static_cast<hipStream_t>(s);
    if (d_counts) PCR_HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)n_classes * sizeof(unsigned long long), st));
    if (n == 0) return PCR_HIP_OK;
    PCR_REQUIRE(d_masks, "filter_classes: null masks");
    PCR_REQUIRE(mask_stride >= n || n_classes == 1, "filter_classes: mask_stride shorter than the point count");
    // the vector part needs 16-byte aligned channels and 4-byte aligned masks; else every point goes one per lane
    bool vec = (reinterpret_cast<uintptr_t>(d_masks) & 3) == 0 && (mask_stride & 3) == 0;
    for (int c = 0; c < t.n_ch; ++c) vec = vec && (reinterpret_cast<uintptr_t>(t.ch[c]) & 15) == 0;
    const uint64_t groups = vec ? n / 4 : 0;
    const dim3 grid(blocks_for(std::max(groups, n - 4 * groups), kSweepThreads)), block(kSweepThreads);
    switch (t.n_ch) {
        case 1: hipLaunchKernelGGL(k_filter_classes<1>, grid, block, 0, st, t, n, groups, d_masks, mask_stride, d_counts); break;
        case 2: hipLaunchKernelGGL(k_filter_classes<2>, grid, block, 0, st, t, n, groups, d_masks, mask_stride, d_counts); break;
        case 3: hipLaunchKernelGGL(k_filter_classes<3>, grid, block, 0, st, t, n, groups, d_masks, mask_stride, d_counts); break;
        case 4: hipLaunchKernelGGL(k_filter_classes<4>, grid, block, 0, st, t, n, groups, d_masks, mask_stride, d_counts); break;
        default: hipLaunchKernelGGL(k_filter_classes<0>, grid, block, 0, st, t, n, groups, d_masks, mask_stride, d_counts); break;
    }
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_engine_touch(pcr_hip_engine* e, const double* d_x, const double* d_y, uint64_t n) {
    PCR_REQUIRE(e, "engine_touch: null engine");
    if (n == 0) return PCR_HIP_OK;
    PCR_REQUIRE(n < ((uint64_t)1 << 40), "engine_touch: too many points in one call");
    PCR_REQUIRE(d_x && d_y, "engine_touch: null coordinate array");
    int prev = -1;
    const bool switched = hipGetDevice(&prev) == hipSuccess && prev != e->device && hipSetDevice(e->device) == hipSuccess;
    hipError_t err;
    {
        ScopedKernelTimer timer(e, "k_touch");
        hipLaunchKernelGGL(k_touch, dim3(blocks_for((n + 1) / 2, kTouchThreads)), dim3(kTouchThreads), 0, e->stream, e->gd, d_x, d_y,
                           n, e->d_touched);
        err = hipGetLastError();
    }
    if (switched) (void)hipSetDevice(prev);
    PCR_HIP_TRY(err);
    return PCR_HIP_OK;
}

}  // extern "C"
