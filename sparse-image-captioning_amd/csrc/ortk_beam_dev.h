// ortk_beam_dev.h — device functions of the beam steps shared by the kernels of ortk_decode.hip and of ortk_decode_joint.hip: the tail of a
// beam step (beam_commit), the wide selection (beam_select_wide) and the penalty list of the grouped steps (pen_build).  Device code
// only; every function is inlined into the kernel that calls it.
#pragma once
#include <type_traits>
#include "ortk_internal.h"

namespace ortk {
namespace {

// ------------------------------------------------------------------------------------------------ beam step
constexpr int MAXB = 8;   // beams kept per thread (>= beam size)

__device__ __forceinline__ double length_pen(int kind, double alpha, int len, double p) {
    if (kind == 1) return p / (pow(5.0 + (double)len, alpha) / pow(6.0, alpha));   // utils/model_utils.py:134-140
    if (kind == 2) return p / (double)len;                                         // utils/model_utils.py:143-146
    return p;
}

// same reductions, in the same order, as log_softmax_kernel (ortk_embed_loss.hip): the fused step is bit-identical to
// log_softmax followed by the unfused step
__device__ __forceinline__ float blk_max(float v, float* sh) {
    v = wave_max(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    float r = sh[0];
    for (int w = 1; w < 4; ++w) r = fmaxf(r, sh[w]);
    return r;
}
__device__ __forceinline__ float blk_sum(float v, float* sh) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    float r = 0.f;
    for (int w = 0; w < 4; ++w) r += sh[w];
    return r;
}

// Arg-best under ortk_better (larger value, lower index on a tie) with a payload that travels with the winner: a list position
// (beam steps), the token's log-prob (fused and truncated sampling), or nothing (NoPayload).
struct NoPayload {};
template <typename T> __device__ __forceinline__ T shfl_xor_payload(T p, int o) {
    if constexpr (std::is_empty_v<T>) return p; else return __shfl_xor(p, o, 64);
}
// the wave's best in every lane
template <typename T>
__device__ __forceinline__ void wave_argbest(float& v, int& i, T& p) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64); const int oi = __shfl_xor(i, o, 64); const T op = shfl_xor_payload(p, o);
        if (ortk_better(ov, oi, v, i)) { v = ov; i = oi; p = op; }
    }
}
__device__ __forceinline__ void wave_argbest(float& v, int& i) { NoPayload none; wave_argbest(v, i, none); }
// the workgroup's best (four waves) in thread 0; red_*: 4 LDS entries each, free again after the caller's next barrier
template <typename T>
__device__ __forceinline__ void blk_argbest(float& v, int& i, T& p, float* red_v, int* red_i, T* red_p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wave_argbest(v, i, p);
    if (lane == 0) { red_v[wave] = v; red_i[wave] = i; if constexpr (!std::is_empty_v<T>) red_p[wave] = p; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w)
            if (ortk_better(red_v[w], red_i[w], v, i)) { v = red_v[w]; i = red_i[w]; if constexpr (!std::is_empty_v<T>) p = red_p[w]; }
}
__device__ __forceinline__ void blk_argbest(float& v, int& i, float* red_v, int* red_i) {
    NoPayload none;
    blk_argbest(v, i, none, red_v, red_i, static_cast<NoPayload*>(nullptr));
}

// STATS: maximum and log-sum-exp of one logit row from its block statistics gs (nblk x {max, sum exp(. - max)}), taken by one wave;
// m[u] is left holding the maximum of block lane + 64 u (-inf past nblk)
__device__ __forceinline__ void stats_row_lse(const float* __restrict__ gs, int nblk, float (&m)[4], float& mx, float& lse) {
    const int lane = threadIdx.x & 63;
    float sb_[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int blk = lane + 64 * u;
        const float2 v2 = blk < nblk ? *reinterpret_cast<const float2*>(gs + 2 * blk) : make_float2(-INFINITY, 0.f);
        m[u] = v2.x; sb_[u] = v2.y;
    }
    mx = wave_max(fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3])));
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) sum += m[u] > -INFINITY ? sb_[u] * __expf(m[u] - mx) : 0.f;
    lse = logf(wave_sum(sum));
}

// The tail of a beam step, shared by beam_step_kernel and beam_step_wide_kernel: the image's b winners (win_v, win_i = parent * V +
// token, in rank order) become its next beams.  row_mx / row_lse: the soft-max statistics of the image's rows; end_slot: b LDS entries.
// Histories, ancestry table, next tokens.  Every copy is spread over the whole workgroup: one thread per beam walking
// its t history entries and t+1 ancestry entries was a chain of ~50 dependent global round trips (the tail of the step
// grew with t and dominated it: 118 us per step at 1 024 images x 5 beams).
__device__ __forceinline__ void beam_commit(const BeamState& st, const float* __restrict__ logp, int t, float scale, const float* win_v,
                                            const int* win_i, const float* row_mx, const float* row_lse, int* end_slot) {
    const int img = blockIdx.x, tid = threadIdx.x;
    const int b = st.b, V = st.V, L = st.L;
    const int cur = t & 1, nxt = cur ^ 1;
    const int64_t row0 = (int64_t)img * b;
    for (int idx = tid; idx < b * t; idx += 256) {
        const int q = idx / t, u = idx - q * t;
        const int parent = win_i[q] / V;
        const int64_t nrow = row0 + q, prow = row0 + parent;
        st.seq[nxt][nrow * L + u] = st.seq[cur][prow * L + u];
        st.tok_lp[nxt][nrow * L + u] = st.tok_lp[cur][prow * L + u];
    }
    for (int idx = tid; idx < b * (t + 1); idx += 256) {
        const int q = idx / (t + 1), u = idx - q * (t + 1);
        const int parent = win_i[q] / V;
        const int64_t srow = t == 0 ? img : row0 + parent;
        const int32_t v = st.kvidx[cur][srow * (t + 1) + u];
        st.kvidx[nxt][(row0 + q) * (t + 2) + u] = v;                                   // ancestors' cache rows
        if (st.uniq) {      // measurement only: is this the first of the image's new beams that references cache row v?
            bool first = true;
            for (int q2 = 0; q2 < q; ++q2) {
                const int64_t s2 = t == 0 ? img : row0 + win_i[q2] / V;
                if (st.kvidx[cur][s2 * (t + 1) + u] == v) first = false;
            }
            if (first) atomicAdd(st.uniq, 1ull);
        }
    }
    if (tid < b) {
        const int q = tid;
        const int ix = win_i[q];
        const int parent = ix / V, tok = ix - parent * V;
        const int64_t nrow = row0 + q, prow = row0 + parent;
        const int64_t srow = t == 0 ? img : prow;
        st.seq[nxt][nrow * L + t] = tok;
        const int pq = t == 0 ? 0 : parent;
        // logit * scale - max with ONE rounding, spelled out: the product has this one use, and the compiler contracted it to an FMA in
        // every instance of both kernels when the narrow one still wrote it as a product and a difference
        st.tok_lp[nxt][nrow * L + t] = __fmaf_rn(logp[srow * st.ldv + tok], scale, -row_mx[pq]) - row_lse[pq];
        st.it[nrow] = tok;
        st.kvidx[nxt][nrow * (t + 2) + t + 1] = (int32_t)(nrow * st.tmax + t + 1);      // this beam's own slot at time t+1
    }
    // finished hypotheses: slots are handed out sequentially per image (insertion order matters for the final stable
    // sort), the copies run in parallel afterwards
    const int cap = b * L;
    if (tid == 0) {
        int cnt = st.done_cnt[img];
        for (int q = 0; q < b; ++q) {
            const int64_t nrow = row0 + q;
            const int ix = win_i[q];
            const int tok = ix - (ix / V) * V;
            float cum = win_v[q];
            const bool end = tok == st.eos || t == L - 1;
            end_slot[q] = -1;
            if (end) {
                if (cnt < cap) {
                    const int64_t base = ((int64_t)img * cap + cnt);
                    end_slot[q] = cnt;
                    st.done_len[base] = t + 1;
                    st.done_p[base] = length_pen(st.length_penalty, st.length_alpha, t + 1, (double)cum);
                    ++cnt;
                }
                cum -= 1000.f;
            }
            st.cum[nrow] = cum;
        }
        st.done_cnt[img] = cnt;
    }
    __syncthreads();          // end_slot, and the histories written above, are visible to the whole workgroup
    for (int idx = tid; idx < b * (t + 1); idx += 256) {
        const int q = idx / (t + 1), u = idx - q * (t + 1);
        if (end_slot[q] < 0) continue;
        const int64_t base = (int64_t)img * cap + end_slot[q], nrow = row0 + q;
        st.done_seq[base * L + u] = st.seq[nxt][nrow * L + u];
        st.done_lp[base * L + u] = st.tok_lp[nxt][nrow * L + u];
    }
}

// FASTEXP (mixed precision only): v_exp_f32 (__expf, ~1 ulp) for the soft-max sum instead of libm's expf — the step is bound by
// the ~20 vector instructions per element of the exact function, not by its one read of the logits (111 -> 60 us per step of
// the 1 024-image beam-5 decode); the fp32 parity mode keeps the exact function (token-exact goldens).
template <bool FAST> __device__ __forceinline__ float exp_sel(float x) { return FAST ? __expf(x) : expf(x); }

// ------------------------------------------------------------------------------------------------ wide beam step (9 .. 32 beams)
// The same contract as beam_step_kernel for any b <= ORTK_MAX_BEAM, as kernel instances of its own (the narrow selection keeps
// its registers and LDS); the tail after the selection is the narrow kernel's, beam_commit.  Selection, one workgroup per image:
//   * row statistics and candidate values by the narrow kernel's expressions in the same mode (blk_max / blk_sum over the
//     256-strided elements, or the generator's 64-logit block statistics under STATS): at b <= 8 the two kernels agree bit for bit;
//     (logit * scale - max is formed with ONE rounding everywhere in this kernel, __fmaf_rn, as log_softmax_kernel's single-use
//     product is contracted; in beam_step_kernel's register-resident rows the product also feeds the row maximum and is rounded
//     first — only at a temperature other than 1 can that last bit differ between the two kernels);
//   * pruning threshold: every row leaves 32 disjoint group maxima (8 lanes x the lane's strided elements, the excluded token
//     left out).  The b largest group maxima seen SO FAR in the image are carried from row to row (a 64-entry rank merge per
//     row); they are b distinct admissible candidates, so the smallest of them is a lower bound of the image's b-th
//     best, and it only rises: row 0 (the best beam) pays ~b ln b list entries, later rows only what can still win;
//   * elements >= the threshold go to an LDS list of WCAP entries; b rounds of block-wide arg-max (value, then flat index)
//     pick the exact winners in rank order;
//   * overflow (massive ties): b passes over the rows, each taking the best candidate that ranks strictly behind the
//     previous winner — exact for any input, no list, no per-thread state.
// No atomically ordered data reaches the result: list positions are arbitrary, the arg-max order is total.
constexpr int WMAXB = ORTK_MAX_BEAM;
constexpr int WCAP = 4096;
struct WideLds {
    float cv[WCAP];
    int ci[WCAP];
    float comb[2][64];        // [.][0..31] the largest group maxima so far (sorted), [.][32..63] the current row's
    float row_mx[WMAXB], row_lse[WMAXB];
    float win_v[WMAXB];
    int win_i[WMAXB];
    float sh_red[4], red_v[4];
    int red_i[4], red_pos[4];
    int cnt;
};

// Diversity penalty of a grouped (diverse) beam step: the tokens the image's earlier groups hold at this position, each with
// pen = fl32(count * lambda) (every copy of a repeated token carries the full count: a lookup takes the first match).  bits: a
// filter of PEN_BITS bits over token & (PEN_BITS - 1) — exact for vocabularies of up to 65 536 tokens — so that the common candidate
// pays one bit test and only a hit walks the list (a wave walks whenever one of its lanes does: at 2 048 bits and 24 entries that was
// every second iteration, profiles/diverse_beam.txt).
constexpr int PEN_BITS = 65536, PEN_WORDS = PEN_BITS / 32;
struct PenLds {
    int tok[ORTK_MAX_BEAM];
    float pen[ORTK_MAX_BEAM];
    unsigned bits[PEN_WORDS];
    int n;
};
// raw: this thread's list entry (threads 0 .. n_pen - 1; -1 = no entry), n_pen <= ORTK_MAX_BEAM - 1; ends with a barrier
__device__ __forceinline__ void pen_build(PenLds& Pn, int raw, int n_pen, float lambda) {
    const int tid = threadIdx.x;
    for (int i = tid; i < PEN_WORDS; i += 256) Pn.bits[i] = 0u;
    if (tid < ORTK_MAX_BEAM) Pn.tok[tid] = tid < n_pen ? raw : -1;
    if (tid == 0) Pn.n = n_pen;
    __syncthreads();
    if (tid < n_pen && raw >= 0) {
        int cnt = 0;
        for (int j = 0; j < n_pen; ++j) cnt += Pn.tok[j] == raw ? 1 : 0;
        Pn.pen[tid] = __fmul_rn((float)cnt, lambda);
        atomicOr(&Pn.bits[(raw >> 5) & (PEN_WORDS - 1)], 1u << (raw & 31));      // (a set: the order of the ORs does not reach the result)
    }
    __syncthreads();
}
// log-prob x of token v minus its penalty (one fp32 subtract; x itself for a token no earlier group holds)
template <bool PEN> __device__ __forceinline__ float pen_sub(const PenLds* Pn, float x, int v) {
    if constexpr (PEN) {
        if (Pn->n > 0 && ((Pn->bits[(v >> 5) & (PEN_WORDS - 1)] >> (v & 31)) & 1u)) {
            const int n = Pn->n;
            for (int i = 0; i < n; ++i) if (Pn->tok[i] == v) return x - Pn->pen[i];
        }
    }
    return x;
}

// block-wide best of (mv, mi) under ortk_better; winner r -> S.win_v[r], S.win_i[r]; `clear`: mp is the winner's list position
__device__ __forceinline__ void wide_argbest(WideLds& S, float mv, int mi, int mp, int r, bool clear) {
    blk_argbest(mv, mi, mp, S.red_v, S.red_i, S.red_pos);
    if (threadIdx.x == 0) {
        S.win_v[r] = mv; S.win_i[r] = mi == 0x7FFFFFFF ? 0 : mi;      // (no candidate left — NaN rows: stay inside the tables)
        if (clear && mp >= 0) S.cv[mp] = -INFINITY, S.ci[mp] = 0x7FFFFFFF;
    }
    __syncthreads();
}

// The b best of the image's nq x V candidates, in rank order, into S.win_v / S.win_i (flat index q * V + v); S.row_mx / S.row_lse
// hold the rows' soft-max statistics when FUSED.  lp0: the image's first logit row; cum (nq values, NULL: 0); prev (token of row
// q at prev[q * prev_stride], NULL: none) is no candidate; gs: the image's first row of block statistics (STATS).
// PEN (grouped steps): every candidate's log-prob first loses the penalty of its token, pen_sub(Pn, ., v); the group maxima behind the
// pruning threshold are maxima of the PENALISED values, so they stay admissible candidates and the threshold stays a lower bound.
template <bool FUSED, int NPT, bool FASTEXP, bool STATS, bool PEN = false>
__device__ __forceinline__ void beam_select_wide(WideLds& S, const float* __restrict__ lp0, int64_t ldv, int nq, int b, int V, float scale,
                                                 const float* __restrict__ cum, const int32_t* __restrict__ prev, int64_t prev_stride,
                                                 const float* __restrict__ gs0, int nblk, const PenLds* Pn = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 32) S.comb[0][tid] = -INFINITY;
    if (tid == 0) S.cnt = 0;
    if (STATS) {
        // one wave per row, the expressions of beam_step_kernel's STATS route
        for (int q = wave; q < nq; q += 4) {
            float m[4], mx, lse;
            stats_row_lse(gs0 + (int64_t)q * nblk * 2, nblk, m, mx, lse);
            if (lane == 0) { S.row_mx[q] = mx; S.row_lse[q] = lse; }
        }
    }
    __syncthreads();
    float zn[NPT > 0 ? NPT : 1];
    if (NPT > 0) {
#pragma unroll
        for (int u = 0; u < NPT; ++u) { const int v = tid + 256 * u; zn[u] = v < V ? lp0[v] : 0.f; }
    }
    for (int q = 0; q < nq; ++q) {
        const float* lp = lp0 + (int64_t)q * ldv;
        float z[NPT > 0 ? NPT : 1];
        if (NPT > 0) {
#pragma unroll
            for (int u = 0; u < NPT; ++u) z[u] = zn[u];
            if (q + 1 < nq) {
                const float* lpn = lp + ldv;
#pragma unroll
                for (int u = 0; u < NPT; ++u) { const int v = tid + 256 * u; zn[u] = v < V ? lpn[v] : 0.f; }
            }
        }
        const float cumq = cum ? cum[q] : 0.f;
        const int pv = prev ? prev[(int64_t)q * prev_stride] : -1;
        float mx = 0.f, lse = 0.f;
        if (STATS) { mx = S.row_mx[q]; lse = S.row_lse[q]; }
        else if (FUSED) {
            float m = -INFINITY, sum = 0.f;
            if (NPT > 0) {
#pragma unroll
                for (int u = 0; u < NPT; ++u) if (tid + 256 * u < V) m = fmaxf(m, z[u] * scale);
                mx = blk_max(m, S.sh_red);
#pragma unroll
                for (int u = 0; u < NPT; ++u) if (tid + 256 * u < V) sum += exp_sel<FASTEXP>(__fmaf_rn(z[u], scale, -mx));
            } else {
                for (int v0 = tid; v0 < V; v0 += 256 * 8) {
                    float x[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) { const int v = v0 + 256 * u; x[u] = v < V ? lp[v] * scale : -INFINITY; }
#pragma unroll
                    for (int u = 0; u < 8; ++u) m = fmaxf(m, x[u]);
                }
                mx = blk_max(m, S.sh_red);
                for (int v0 = tid; v0 < V; v0 += 256 * 8) {
                    float x[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) { const int v = v0 + 256 * u; x[u] = v < V ? lp[v] : 0.f; }
#pragma unroll
                    for (int u = 0; u < 8; ++u) if (v0 + 256 * u < V) sum += exp_sel<FASTEXP>(__fmaf_rn(x[u], scale, -mx));
                }
            }
            sum = blk_sum(sum, S.sh_red);
            lse = logf(sum);
            if (tid == 0) { S.row_mx[q] = mx; S.row_lse[q] = lse; }
        }
        // candidate values and this thread's maximum
        float tm = -INFINITY;
        if (NPT > 0) {
#pragma unroll
            for (int u = 0; u < NPT; ++u) {
                const int v = tid + 256 * u;
                const bool ok = v < V && v != pv;
                z[u] = ok ? cumq + pen_sub<PEN>(Pn, __fmaf_rn(z[u], scale, -mx) - lse, v) : -INFINITY;
                tm = fmaxf(tm, z[u]);
            }
        } else {
            for (int v0 = tid; v0 < V; v0 += 256 * 8) {
                float x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int v = v0 + 256 * u; x[u] = v < V ? lp[v] : 0.f; }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int v = v0 + 256 * u;
                    if (v >= V || v == pv) continue;
                    tm = fmaxf(tm, cumq + pen_sub<PEN>(Pn, FUSED ? __fmaf_rn(x[u], scale, -mx) - lse : x[u], v));
                }
            }
        }
#pragma unroll
        for (int o2 = 4; o2 > 0; o2 >>= 1) tm = fmaxf(tm, __shfl_xor(tm, o2, 64));
        float* cb = S.comb[q & 1];
        if ((lane & 7) == 0) cb[32 + wave * 8 + (lane >> 3)] = tm;
        __syncthreads();
        // rank of the 64 maxima (the carried 32 and this row's 32), every wave for itself: lane j ranks entry j
        const float mine = cb[lane];
        int rank = 0;
        for (int j = 0; j < 64; ++j) { const float o = cb[j]; rank += (o > mine || (o == mine && j < lane)) ? 1 : 0; }
        const float tau = __shfl(mine, __ffsll((unsigned long long)__ballot(rank == b - 1)) - 1, 64);
        if (rank < 32) S.comb[(q + 1) & 1][rank] = mine;          // (all four waves store the same values)
        if (NPT > 0) {
#pragma unroll
            for (int u = 0; u < NPT; ++u) {
                const int v = tid + 256 * u;
                if (v < V && v != pv && z[u] >= tau) {
                    const int pos = atomicAdd(&S.cnt, 1);
                    if (pos < WCAP) { S.cv[pos] = z[u]; S.ci[pos] = q * V + v; }
                }
            }
        } else {
            for (int v0 = tid; v0 < V; v0 += 256 * 8) {
                float x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int v = v0 + 256 * u; x[u] = v < V ? lp[v] : 0.f; }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int v = v0 + 256 * u;
                    if (v >= V || v == pv) continue;
                    const float zz = cumq + pen_sub<PEN>(Pn, FUSED ? __fmaf_rn(x[u], scale, -mx) - lse : x[u], v);
                    if (zz >= tau) {
                        const int pos = atomicAdd(&S.cnt, 1);
                        if (pos < WCAP) { S.cv[pos] = zz; S.ci[pos] = q * V + v; }
                    }
                }
            }
        }
    }
    __syncthreads();
    const int n = S.cnt;                 // block-uniform
    if (n <= WCAP) {
        for (int r = 0; r < b; ++r) {
            float mv = -INFINITY; int mi = 0x7FFFFFFF, mp = -1;
            for (int i = tid; i < n; i += 256) {
                const float v = S.cv[i]; const int ix = S.ci[i];
                if (ortk_better(v, ix, mv, mi)) { mv = v; mi = ix; mp = i; }
            }
            wide_argbest(S, mv, mi, mp, r, true);
        }
        return;
    }
    // overflow: winner r = the best candidate that ranks strictly behind winner r - 1
    float lv = INFINITY; int li = -1;
    for (int r = 0; r < b; ++r) {
        float mv = -INFINITY; int mi = 0x7FFFFFFF;
        for (int q = 0; q < nq; ++q) {
            const float* lp = lp0 + (int64_t)q * ldv;
            const float cumq = cum ? cum[q] : 0.f;
            const int pv = prev ? prev[(int64_t)q * prev_stride] : -1;
            const float mx = FUSED ? S.row_mx[q] : 0.f, lse = FUSED ? S.row_lse[q] : 0.f;
            for (int v0 = tid; v0 < V; v0 += 256 * 8) {
                float x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int v = v0 + 256 * u; x[u] = v < V ? lp[v] : 0.f; }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int v = v0 + 256 * u;
                    if (v >= V || v == pv) continue;
                    const float zz = cumq + pen_sub<PEN>(Pn, FUSED ? __fmaf_rn(x[u], scale, -mx) - lse : x[u], v);
                    const int ix = q * V + v;
                    if (ortk_better(lv, li, zz, ix) && ortk_better(zz, ix, mv, mi)) { mv = zz; mi = ix; }
                }
            }
        }
        wide_argbest(S, mv, mi, -1, r, false);
        lv = S.win_v[r]; li = S.win_i[r];
    }
}

}  // namespace
}  // namespace ortk
