// ortk_select.hip — magnitude-pruning mask selection on the device: the n_drop smallest criteria of a group of arena segments get
// mask 0, the group's other positions 1 (pruning/prune.py:271-283,330-365: cat + topk + scatter), without a sort.
//
// The criterion c >= 0 (|w|, or |(w - mean_s) / std_s| per segment), so its fp32 bit pattern with the sign cleared is a monotone
// uint32 key: -0.0 ties with +0.0, denormals are ordinary keys, NaN ranks above +inf.  An MSB-first radix select (4 passes of 8
// bits) finds each group's threshold key T and the number r of entries EQUAL to T that still have to go; among those the lowest
// positions in group order (segments as listed, flat index inside a segment) are dropped.
//
//   init                      state[g] = {prefix 0, k = n_drop[g]}, hist = 0
//   4 x { hist pass           one workgroup per chunk: digit histogram of the keys matching the prefix, 256 LDS bins, integer
//                             atomics into hist[g][256]
//         pick                one wave per group: smallest digit whose cumulative count reaches k; prefix |= digit, k -= below }
//   tie pass                  per wave range of a chunk: number of keys == T
//   scan                      one wave per group: exclusive scan of those counts in chunk order
//   write                     mask = key < T ? 0 : (key == T and tie rank < r) ? 0 : 1, 16 bytes per lane where aligned
//
// A chunk (segment, start, length) belongs to one workgroup of four waves; wave v owns the v-th quarter of it (a contiguous
// range), so the tie rank needs wave scans only.  Kind 1 recomputes c in every pass from the per-segment {mean, std}: fp64 sums
// in a fixed order (thread-sequential, wave tree, four waves, then one wave per segment over the chunk partials), two passes
// (mean, then the squared deviations), both rounded to fp32 — no floating-point atomics, so two runs give the same bits.
// Nothing outside the listed segments is read or written, no launch depends on the host, everything is on the caller's stream.
#include "ortk_common.h"

namespace {

constexpr int SEL_WG = 256;            // four waves per chunk
constexpr int SEL_WAVES = SEL_WG / ORTK_WAVE;
constexpr int SEL_MAX_SEGMENTS = 4096;

struct sel_tables {
    const int64_t *seg_offset, *seg_numel, *seg_group, *chunk_seg, *chunk_start, *chunk_len;
};
struct sel_ws {
    uint32_t* state;       // [n_groups][2]  {prefix, k}; after the fourth pick {T, r}
    uint32_t* hist;        // [n_groups][256]
    uint32_t* tie;         // [n_chunks][SEL_WAVES]  counts, then exclusive ranks
    double* partial;       // kind 1: [n_chunks]
    double* mean64;        // kind 1: [n_segments]
    float* stat;           // kind 1: [n_segments][2]  {mean, std} as fp32
};

static size_t sel_up16(size_t b) { return (b + 15) & ~(size_t)15; }
static size_t sel_layout(int32_t n_segments, int32_t n_groups, int32_t n_chunks, int32_t kind, void* base, sel_ws* out) {
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += sel_up16(bytes); return base ? (char*)base + o : (char*)nullptr; };
    sel_ws w{};
    w.state = (uint32_t*)take((size_t)n_groups * 2 * sizeof(uint32_t));
    w.hist = (uint32_t*)take((size_t)n_groups * 256 * sizeof(uint32_t));
    w.tie = (uint32_t*)take((size_t)n_chunks * SEL_WAVES * sizeof(uint32_t));
    if (kind == 1) {
        w.partial = (double*)take((size_t)n_chunks * sizeof(double));
        w.mean64 = (double*)take((size_t)n_segments * sizeof(double));
        w.stat = (float*)take((size_t)n_segments * 2 * sizeof(float));
    }
    if (out) *out = w;
    return off;
}

// ---- the range of a chunk that one wave walks, four consecutive elements per lane and step
struct wave_range {
    int64_t lo, hi;        // arena indices
    bool vec;              // lo is a multiple of 4: full quads move as 16 bytes
    int seg;
};
__device__ __forceinline__ wave_range sel_range(const sel_tables& t, int chunk) {
    const int seg = (int)t.chunk_seg[chunk];
    const int64_t base = t.seg_offset[seg] + t.chunk_start[chunk], len = t.chunk_len[chunk];
    const int64_t q = (((len + SEL_WAVES - 1) / SEL_WAVES) + 3) & ~(int64_t)3;
    const int v = threadIdx.x / ORTK_WAVE;
    wave_range r;
    r.lo = base + (v * q < len ? v * q : len);
    r.hi = base + ((v + 1) * q < len ? (v + 1) * q : len);
    r.vec = (base & 3) == 0;
    r.seg = seg;
    return r;
}
// elements i .. i+3 clipped to hi; returns the number of valid ones
__device__ __forceinline__ int sel_load(const float* __restrict__ w, int64_t i, const wave_range& r, float (&x)[4]) {
    const int64_t left = r.hi - i;
    const int n = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
    if (n == 4 && r.vec) {
        const float4 q = *reinterpret_cast<const float4*>(w + i);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = j < n ? w[i + j] : 0.f;
    }
    return n;
}
template <int KIND>
__device__ __forceinline__ uint32_t sel_key(float x, float mean, float sd) {
    const float c = KIND == 0 ? x : (x - mean) / sd;       // a true division, as torch's element-wise expression
    return __float_as_uint(c) & 0x7FFFFFFFu;
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    const int lane = threadIdx.x & (ORTK_WAVE - 1);
#pragma unroll
    for (int o = 1; o < ORTK_WAVE; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, ORTK_WAVE);
        if (lane >= o) v += u;
    }
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, ORTK_WAVE);
    return v;
}

__global__ __launch_bounds__(256) void sel_init_kernel(sel_ws ws, const int64_t* __restrict__ n_drop, int n_groups) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (int64_t)n_groups * 256) ws.hist[i] = 0u;
    if (i < n_groups) { ws.state[2 * i] = 0u; ws.state[2 * i + 1] = (uint32_t)n_drop[i]; }
}

// ---- kind 1 statistics.  PHASE 0: sum of x;  PHASE 1: sum of (x - mean)^2, both fp64, one partial per chunk
template <int PHASE>
__global__ __launch_bounds__(SEL_WG) void sel_stat_chunk_kernel(const float* __restrict__ w, sel_tables t, sel_ws ws) {
    __shared__ double sh[SEL_WAVES];
    const int chunk = blockIdx.x, lane = threadIdx.x & (ORTK_WAVE - 1);
    const wave_range r = sel_range(t, chunk);
    const double mean = PHASE ? ws.mean64[r.seg] : 0.0;
    double acc = 0.0;
    for (int64_t p = r.lo; p < r.hi; p += ORTK_WAVE * 4) {
        float x[4];
        const int n = sel_load(w, p + lane * 4, r, x);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) { const double d = (double)x[j] - mean; acc += PHASE ? d * d : d; }
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) sh[threadIdx.x / ORTK_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) ws.partial[chunk] = ((sh[0] + sh[1]) + (sh[2] + sh[3]));
}
// one wave per segment: the chunk partials of the segment, lane l takes chunks l, l+64, ... in ascending order
template <int PHASE>
__global__ __launch_bounds__(ORTK_WAVE) void sel_stat_seg_kernel(sel_tables t, sel_ws ws, int n_chunks) {
    const int seg = blockIdx.x, lane = threadIdx.x;
    double acc = 0.0;
    for (int c = lane; c < n_chunks; c += ORTK_WAVE)
        if ((int)t.chunk_seg[c] == seg) acc += ws.partial[c];
    acc = wave_sum_f64(acc);
    if (lane == 0) {
        const double n = (double)t.seg_numel[seg];
        if (PHASE == 0) { ws.mean64[seg] = acc / n; ws.stat[2 * seg] = (float)(acc / n); }
        else ws.stat[2 * seg + 1] = (float)sqrt(acc / n);
    }
}

// ---- one radix pass: histogram of digit `shift` over the keys whose higher digits equal the group's prefix
template <int KIND>
__global__ __launch_bounds__(SEL_WG) void sel_hist_kernel(const float* __restrict__ w, sel_tables t, sel_ws ws, int shift) {
    __shared__ uint32_t bins[256];
    const int chunk = blockIdx.x, lane = threadIdx.x & (ORTK_WAVE - 1);
    bins[threadIdx.x] = 0u;
    const wave_range r = sel_range(t, chunk);
    const int g = (int)t.seg_group[r.seg];
    const uint32_t prefix = ws.state[2 * g];
    const uint32_t himask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
    const float mean = KIND ? ws.stat[2 * r.seg] : 0.f, sd = KIND ? ws.stat[2 * r.seg + 1] : 1.f;
    __syncthreads();
    // consecutive keys often share the digit (the first pass sees a handful of exponents): a lane adds a run at once
    uint32_t run_digit = 0u, run = 0u;
    for (int64_t p = r.lo; p < r.hi; p += ORTK_WAVE * 4) {
        float x[4];
        const int n = sel_load(w, p + lane * 4, r, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t key = sel_key<KIND>(x[j], mean, sd);
            if (j < n && (key & himask) == prefix) {
                const uint32_t d = (key >> shift) & 255u;
                if (d != run_digit) {
                    if (run) atomicAdd(&bins[run_digit], run);
                    run_digit = d; run = 0u;
                }
                ++run;
            }
        }
    }
    if (run) atomicAdd(&bins[run_digit], run);
    __syncthreads();
    const uint32_t b = bins[threadIdx.x];
    if (b) atomicAdd(&ws.hist[(size_t)g * 256 + threadIdx.x], b);
}

// one wave per group: lane l holds bins 4l .. 4l+3.  The smallest digit whose cumulative count reaches k is the next digit of the
// threshold key; k becomes the rank inside that digit's class.  k == 0 (nothing to drop) stays 0 with digit 0.  The bins are
// cleared for the next pass.
__global__ __launch_bounds__(ORTK_WAVE) void sel_pick_kernel(sel_ws ws, int shift) {
    const int g = blockIdx.x, lane = threadIdx.x;
    uint32_t* h = ws.hist + (size_t)g * 256 + lane * 4;
    const uint4 b = *reinterpret_cast<const uint4*>(h);
    *reinterpret_cast<uint4*>(h) = make_uint4(0u, 0u, 0u, 0u);
    const uint32_t k = ws.state[2 * g + 1];
    const uint32_t c[4] = {b.x, b.y, b.z, b.w};
    const uint32_t sum = b.x + b.y + b.z + b.w;
    const uint32_t incl = wave_incl_scan(sum);
    const unsigned long long reach = __ballot(incl >= k);
    // (a table with n_drop above the group's size never reaches k: the last digit is taken, nothing is read out of bounds)
    const int owner = reach ? __ffsll((long long)reach) - 1 : ORTK_WAVE - 1;
    if (lane == owner) {
        uint32_t below = incl - sum;
        int j = 0;
        while (j < 3 && below + c[j] < k) { below += c[j]; ++j; }
        ws.state[2 * g] |= (uint32_t)(lane * 4 + j) << shift;
        ws.state[2 * g + 1] = k > below ? k - below : 0u;
    }
}

// ---- ties: how many keys of each wave range equal the threshold key
template <int KIND>
__global__ __launch_bounds__(SEL_WG) void sel_tie_kernel(const float* __restrict__ w, sel_tables t, sel_ws ws) {
    const int chunk = blockIdx.x, lane = threadIdx.x & (ORTK_WAVE - 1);
    const wave_range r = sel_range(t, chunk);
    const int g = (int)t.seg_group[r.seg];
    const uint32_t T = ws.state[2 * g];
    const float mean = KIND ? ws.stat[2 * r.seg] : 0.f, sd = KIND ? ws.stat[2 * r.seg + 1] : 1.f;
    int cnt = 0;
    for (int64_t p = r.lo; p < r.hi; p += ORTK_WAVE * 4) {
        float x[4];
        const int n = sel_load(w, p + lane * 4, r, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) cnt += (j < n && sel_key<KIND>(x[j], mean, sd) == T) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, ORTK_WAVE);
    if (lane == 0) ws.tie[(size_t)chunk * SEL_WAVES + threadIdx.x / ORTK_WAVE] = (uint32_t)cnt;
}

// one wave per group: the counts of the group's wave ranges, in chunk order, become exclusive ranks
__global__ __launch_bounds__(ORTK_WAVE) void sel_scan_kernel(sel_tables t, sel_ws ws, int n_chunks) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int64_t n = (int64_t)n_chunks * SEL_WAVES;
    uint32_t carry = 0u;
    for (int64_t i0 = 0; i0 < n; i0 += ORTK_WAVE) {
        const int64_t i = i0 + lane;
        const bool mine = i < n && (int)t.seg_group[t.chunk_seg[i / SEL_WAVES]] == g;
        const uint32_t v = mine ? ws.tie[i] : 0u;
        const uint32_t incl = wave_incl_scan(v);
        if (mine) ws.tie[i] = carry + incl - v;
        carry += __shfl(incl, ORTK_WAVE - 1, ORTK_WAVE);
    }
}

// ---- the mask
template <int KIND>
__global__ __launch_bounds__(SEL_WG) void sel_write_kernel(const float* __restrict__ w, float* __restrict__ mask, sel_tables t, sel_ws ws) {
    const int chunk = blockIdx.x, lane = threadIdx.x & (ORTK_WAVE - 1);
    const wave_range r = sel_range(t, chunk);
    const int g = (int)t.seg_group[r.seg];
    const uint32_t T = ws.state[2 * g], todrop = ws.state[2 * g + 1];
    const float mean = KIND ? ws.stat[2 * r.seg] : 0.f, sd = KIND ? ws.stat[2 * r.seg + 1] : 1.f;
    uint32_t rank0 = ws.tie[(size_t)chunk * SEL_WAVES + threadIdx.x / ORTK_WAVE];     // ties before this step, in group order
    for (int64_t p = r.lo; p < r.hi; p += ORTK_WAVE * 4) {
        float x[4];
        const int64_t i = p + lane * 4;
        const int n = sel_load(w, i, r, x);
        uint32_t key[4];
        uint32_t ties = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            key[j] = sel_key<KIND>(x[j], mean, sd);
            ties += (j < n && key[j] == T) ? 1u : 0u;
        }
        uint32_t rank = todrop;                          // (a tie at rank >= todrop is kept)
        if (rank0 < todrop && __ballot(ties > 0u)) {     // wave-uniform: once every tie left is kept, no ranks are needed
            const uint32_t incl = wave_incl_scan(ties);
            rank = rank0 + incl - ties;
            rank0 += __shfl(incl, ORTK_WAVE - 1, ORTK_WAVE);
        }
        float m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bool drop = key[j] < T;
            if (j < n && key[j] == T) { drop = rank < todrop; ++rank; }
            m[j] = drop ? 0.f : 1.f;
        }
        if (n == 4 && r.vec) {
            *reinterpret_cast<float4*>(mask + i) = make_float4(m[0], m[1], m[2], m[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) mask[i + j] = m[j];
        }
    }
}

template <int KIND>
int sel_run(const float* w, float* mask, const sel_tables& t, const sel_ws& ws, const int64_t* n_drop, int n_segments, int n_groups,
            int n_chunks, hipStream_t s) {
    hipLaunchKernelGGL(sel_init_kernel, dim3(n_groups), dim3(256), 0, s, ws, n_drop, n_groups);
    ORTK_CHECK_LAUNCH();
    if (KIND == 1) {
        hipLaunchKernelGGL(sel_stat_chunk_kernel<0>, dim3(n_chunks), dim3(SEL_WG), 0, s, w, t, ws);
        hipLaunchKernelGGL(sel_stat_seg_kernel<0>, dim3(n_segments), dim3(ORTK_WAVE), 0, s, t, ws, n_chunks);
        hipLaunchKernelGGL(sel_stat_chunk_kernel<1>, dim3(n_chunks), dim3(SEL_WG), 0, s, w, t, ws);
        hipLaunchKernelGGL(sel_stat_seg_kernel<1>, dim3(n_segments), dim3(ORTK_WAVE), 0, s, t, ws, n_chunks);
        ORTK_CHECK_LAUNCH();
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(sel_hist_kernel<KIND>, dim3(n_chunks), dim3(SEL_WG), 0, s, w, t, ws, shift);
        hipLaunchKernelGGL(sel_pick_kernel, dim3(n_groups), dim3(ORTK_WAVE), 0, s, ws, shift);
        ORTK_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(sel_tie_kernel<KIND>, dim3(n_chunks), dim3(SEL_WG), 0, s, w, t, ws);
    hipLaunchKernelGGL(sel_scan_kernel, dim3(n_groups), dim3(ORTK_WAVE), 0, s, t, ws, n_chunks);
    hipLaunchKernelGGL(sel_write_kernel<KIND>, dim3(n_chunks), dim3(SEL_WG), 0, s, w, mask, t, ws);
    ORTK_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" size_t ortk_mask_select_workspace_bytes(int32_t n_segments, int32_t n_groups, int32_t n_chunks, int32_t kind) {
    if (n_segments <= 0 || n_groups <= 0 || n_chunks <= 0 || kind < 0 || kind > 1) return 0;
    return sel_layout(n_segments, n_groups, n_chunks, kind, nullptr, nullptr);
}

extern "C" int ortk_mask_select(const float* w, float* mask, const int64_t* seg_offset, const int64_t* seg_numel,
                                const int64_t* seg_group, const int64_t* chunk_seg, const int64_t* chunk_start,
                                const int64_t* chunk_len, const int64_t* n_drop, int32_t n_segments, int32_t n_groups,
                                int32_t n_chunks, int32_t kind, void* workspace, size_t workspace_bytes, ortk_stream stream) {
    if (!w || !mask || !seg_offset || !seg_numel || !seg_group || !chunk_seg || !chunk_start || !chunk_len || !n_drop || !workspace)
        return ORTK_EINVAL;
    if (n_segments <= 0 || n_groups <= 0 || n_chunks <= 0 || n_segments > SEL_MAX_SEGMENTS || kind < 0 || kind > 1) return ORTK_EINVAL;
    if (((uintptr_t)workspace & 15) != 0) return ORTK_EINVAL;
    sel_ws ws;
    if (workspace_bytes < sel_layout(n_segments, n_groups, n_chunks, kind, workspace, &ws)) return ORTK_EINVAL;
    const sel_tables t{seg_offset, seg_numel, seg_group, chunk_seg, chunk_start, chunk_len};
    return kind == 0 ? sel_run<0>(w, mask, t, ws, n_drop, n_segments, n_groups, n_chunks, ortk_s(stream))
                     : sel_run<1>(w, mask, t, ws, n_drop, n_segments, n_groups, n_chunks, ortk_s(stream));
}
