// ortk_decode.hip — on-device bookkeeping of greedy / multinomial / beam-search decoding.
//
// Replaces the host loops of CaptionModel.batch_beam_search (models/caption_model.py:56-111,151-226) and of
// CachedTransformerBase._generate_captions (models/transformer.py:507-561).  The reference does, per step, a full
// sort of b*V candidates per image, a Python loop over images x beams with two .item() syncs each, a torch.cat of
// the (N,b,t,V) log-prob history and an index_select of all 24 cache tensors.  Here:
//   * one workgroup per image selects the b best of b*V candidates (per-thread top lists -> LDS -> b rounds of
//     block arg-max), in descending order like the sort;
//   * histories are (N*b, L) token / token-log-prob tables re-ordered by parent (ping-pong buffers);
//   * the self-attention KV cache is NEVER moved: each beam carries a table of the physical cache rows of its
//     ancestors (kvidx), re-threaded by parent pointer each step; cross-attention K/V exist once per image;
//   * finished hypotheses go to a per-image list; the final stable top-b by (length-penalised) score runs on
//     device too.  No host synchronisation anywhere in the 18 steps.
#include "ortk_beam_dev.h"

namespace ortk {
namespace {

__global__ void kv_append_kernel(const float* __restrict__ qkv, void* __restrict__ ck, void* __restrict__ cv, int kvdt, int64_t rows,
                                 int d, int row_mult, int tmax, int t) {
    const int64_t n = rows * d;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / d;
        const int c = (int)(i - r * d);
        const int64_t dst = ((r * row_mult) * tmax + t) * d + c;
        st_elem(ck, dst, kvdt, qkv[r * 3 * d + d + c]);
        st_elem(cv, dst, kvdt, qkv[r * 3 * d + 2 * d + c]);
    }
}

__global__ void fill_i64_kernel(int64_t* p, int64_t n, int64_t v) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = v;
}
__global__ void fill_i32_kernel(int32_t* p, int64_t n, int32_t v) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = v;
}
__global__ void decode_poison_kernel(const int32_t* __restrict__ status, int64_t* __restrict__ seq, float* __restrict__ lp, float* __restrict__ score,
                                     int64_t nseq, int64_t nscore) {
    if (*status == 0) return;
    const float nan = __builtin_nanf("");
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nseq; i += (int64_t)gridDim.x * 256) { seq[i] = 0; lp[i] = nan; }
    if (score) for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nscore; i += (int64_t)gridDim.x * 256) score[i] = nan;
}
__global__ void kvidx_init_kernel(int32_t* p, int64_t rows, int row_mult, int tmax) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rows; i += (int64_t)gridDim.x * 256)
        p[i] = (int32_t)(i * row_mult * tmax);
}

// `logp` holds raw generator logits; the row's log-soft-max (of logits * scale) is taken here — max, sum and
// candidate scan are three strided passes over the row (the 2nd and 3rd hit L2), with 8 independent loads in flight
// per thread.  Saves the separate log-soft-max launch (read + write of rows x V fp32 per step).
// STATS (scale = 1): the generator GEMM has left {max, sum exp(. - max)} of every block of 64 logits (st.gstats).
// The row's log-sum-exp comes from those 2 x 158 floats; the (b + 1)-th largest block maximum is a lower bound of the row's
// b-th best admissible element (block maxima are elements of distinct blocks, at most one of them is the token the decoding
// constraint excludes), so only the b + 1 blocks at or above it are read: 1.6 KB of a 40-KB logit row.
template <int NPT, bool FASTEXP = false, bool STATS = false>
__global__ __launch_bounds__(256) void beam_step_kernel(BeamState st, const float* __restrict__ logp, int t, float scale) {
    __shared__ float sv[256 * MAXB];
    __shared__ float sh_red[4];
    __shared__ float row_mx[MAXB], row_lse[MAXB];
    __shared__ int si[256 * MAXB];
    __shared__ float red_v[4];
    __shared__ int red_i[4], red_pos[4];
    __shared__ float win_v[MAXB];
    __shared__ int win_i[MAXB], end_slot[MAXB];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = st.b, V = st.V, L = st.L;
    const int nq = t == 0 ? 1 : b;
    const int cur = t & 1;

    float bv[MAXB];
    int bi[MAXB];
#pragma unroll
    for (int k = 0; k < MAXB; ++k) { bv[k] = -INFINITY; bi[k] = 0x7FFFFFFF; }
    bool staged = false;     // true once sv / si hold the candidates (fast path); block-uniform
    if (STATS) {
        // one WAVE per row (rows q = wave, wave + 4): the 158 block statistics sit 3 per lane, every reduction is a wave
        // reduction and the b + 1 block reads of a row are issued together — the rows of an image proceed in parallel instead
        // of as a chain of block-wide barriers and dependent loads
        __shared__ int cand_cnt2;
        for (int k = 0; k < MAXB; ++k) { sv[tid * MAXB + k] = -INFINITY; si[tid * MAXB + k] = 0x7FFFFFFF; }
        if (tid == 0) cand_cnt2 = 0;
        __syncthreads();
        const int nblk = st.nblk;                     // <= 256: at most 4 blocks per lane
        const int want = min(b + 1, nblk);            // blocks to read per row
        for (int q = wave; q < nq; q += 4) {
            const int64_t srow = t == 0 ? (int64_t)img : (int64_t)img * b + q;
            float m[4], mx, lse;
            stats_row_lse(st.gstats + srow * nblk * 2, nblk, m, mx, lse);
            const float cum = t == 0 ? 0.f : st.cum[(int64_t)img * b + q];
            const int prev = (st.decoding_constraint && t > 0) ? st.seq[cur][((int64_t)img * b + q) * L + t - 1] : -1;
            if (lane == 0) { row_mx[q] = mx; row_lse[q] = lse; }
            // the `want` largest block maxima, one wave arg-max round each (ties: the lower block)
            int selb[MAXB + 1];
            float tau_raw = -INFINITY;
#pragma unroll
            for (int r = 0; r < MAXB + 1; ++r) {
                selb[r] = -1;
                if (r < want) {
                    float bv_ = m[0]; int bb = lane;
#pragma unroll
                    for (int u = 1; u < 4; ++u) if (m[u] > bv_) { bv_ = m[u]; bb = lane + 64 * u; }
                    wave_argbest(bv_, bb);
                    selb[r] = bb; tau_raw = bv_;
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (bb == lane + 64 * u) m[u] = -INFINITY;      // (never selected twice)
                }
            }
            const float tau = cum + ((tau_raw - mx) - lse);
            float zv[MAXB + 1];
#pragma unroll
            for (int r = 0; r < MAXB + 1; ++r) {
                const int v = selb[r] * 64 + lane;
                zv[r] = (selb[r] >= 0 && v < V) ? logp[srow * st.ldv + v] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < MAXB + 1; ++r) {
                const int v = selb[r] * 64 + lane;
                if (selb[r] >= 0 && v < V && v != prev) {
                    const float z = cum + ((zv[r] - mx) - lse);
                    if (z >= tau) {
                        const int pos = atomicAdd(&cand_cnt2, 1);
                        if (pos < 256 * MAXB) { sv[pos] = z; si[pos] = q * V + v; }
                    }
                }
            }
        }
        __syncthreads();
        staged = cand_cnt2 <= 256 * MAXB;          // (massive ties: the exact per-thread lists below)
        __syncthreads();
    } else if (NPT > 0) {
        // Register-resident rows: each thread holds its NPT strided elements of a row (ONE memory round trip per row, the
        // next row's loads are issued before the current row is reduced); max and sum-exp run in the element order of
        // log_softmax_kernel.  Candidate selection without per-thread sorted lists (their insertion network ran for almost
        // every element because some lane of the wave always inserted): per row, tau = the b-th largest of the 16
        // half-wave-quarter maxima is a lower bound of the row's b-th best, so only the handful of elements >= tau go to
        // the LDS candidate list; the b block-wide arg-max rounds below then pick the exact top-b (value, then index).
        __shared__ float gmax[16];
        __shared__ int cand_cnt;
        for (int k = 0; k < MAXB; ++k) { sv[tid * MAXB + k] = -INFINITY; si[tid * MAXB + k] = 0x7FFFFFFF; }
        if (tid == 0) cand_cnt = 0;
        float zn[NPT > 0 ? NPT : 1];
        {
            const float* lp0 = logp + (t == 0 ? (int64_t)img : (int64_t)img * b) * st.ldv;
#pragma unroll
            for (int u = 0; u < NPT; ++u) { const int v = tid + 256 * u; zn[u] = v < V ? lp0[v] : 0.f; }
        }
        for (int q = 0; q < nq; ++q) {
            float z[NPT > 0 ? NPT : 1];
#pragma unroll
            for (int u = 0; u < NPT; ++u) z[u] = zn[u];
            if (q + 1 < nq) {
                const float* lpn = logp + ((int64_t)img * b + q + 1) * st.ldv;
#pragma unroll
                for (int u = 0; u < NPT; ++u) { const int v = tid + 256 * u; zn[u] = v < V ? lpn[v] : 0.f; }
            }
            const float cum = t == 0 ? 0.f : st.cum[(int64_t)img * b + q];
            const int prev = (st.decoding_constraint && t > 0) ? st.seq[cur][((int64_t)img * b + q) * L + t - 1] : -1;
            float m = -INFINITY;
#pragma unroll
            for (int u = 0; u < NPT; ++u) if (tid + 256 * u < V) m = fmaxf(m, z[u] * scale);
            const float mx = blk_max(m, sh_red);
            float sum = 0.f;
#pragma unroll
            for (int u = 0; u < NPT; ++u) if (tid + 256 * u < V) sum += exp_sel<FASTEXP>(z[u] * scale - mx);
            sum = blk_sum(sum, sh_red);
            const float lse = logf(sum);
            if (tid == 0) { row_mx[q] = mx; row_lse[q] = lse; }
            float tm = -INFINITY;
#pragma unroll
            for (int u = 0; u < NPT; ++u) {
                const int v = tid + 256 * u;
                const bool ok = v < V && v != prev;
                z[u] = ok ? cum + ((z[u] * scale - mx) - lse) : -INFINITY;
                tm = fmaxf(tm, z[u]);
            }
#pragma unroll
            for (int o2 = 8; o2 > 0; o2 >>= 1) tm = fmaxf(tm, __shfl_xor(tm, o2, 64));
            __syncthreads();                       // gmax of the previous row fully consumed
            if ((lane & 15) == 0) gmax[wave * 4 + (lane >> 4)] = tm;
            __syncthreads();
            float gm[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) gm[u] = gmax[u];
            float tau = -INFINITY;
            for (int r = 0; r < b; ++r) {
                float best = gm[0];
#pragma unroll
                for (int u = 1; u < 16; ++u) best = fmaxf(best, gm[u]);
                tau = best;
                bool removed = false;
#pragma unroll
                for (int u = 0; u < 16; ++u) if (!removed && gm[u] == best) { gm[u] = -INFINITY; removed = true; }
            }
#pragma unroll
            for (int u = 0; u < NPT; ++u) {
                const int v = tid + 256 * u;
                if (v < V && v != prev && z[u] >= tau) {
                    const int pos = atomicAdd(&cand_cnt, 1);
                    if (pos < 256 * MAXB) { sv[pos] = z[u]; si[pos] = q * V + v; }
                }
            }
        }
        __syncthreads();
        staged = cand_cnt <= 256 * MAXB;           // overflow (massive ties): redo with the exact per-thread lists
        __syncthreads();
    }
    if (!staged) {
    for (int q = 0; q < nq; ++q) {
        const int64_t srow = t == 0 ? img : (int64_t)img * b + q;
        const float* lp = logp + srow * st.ldv;
        const float cum = t == 0 ? 0.f : st.cum[(int64_t)img * b + q];
        const int prev = (st.decoding_constraint && t > 0) ? st.seq[cur][((int64_t)img * b + q) * L + t - 1] : -1;
        float m = -INFINITY;
        for (int v0 = tid; v0 < V; v0 += 256 * 8) {
            float z[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int v = v0 + 256 * u; z[u] = v < V ? lp[v] * scale : -INFINITY; }
#pragma unroll
            for (int u = 0; u < 8; ++u) m = fmaxf(m, z[u]);
        }
        const float mx = blk_max(m, sh_red);
        float sum = 0.f;
        for (int v0 = tid; v0 < V; v0 += 256 * 8) {
            float z[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int v = v0 + 256 * u; z[u] = v < V ? lp[v] : 0.f; }
#pragma unroll
            for (int u = 0; u < 8; ++u) if (v0 + 256 * u < V) sum += expf(z[u] * scale - mx);
        }
        sum = blk_sum(sum, sh_red);
        const float lse = logf(sum);
        if (tid == 0) { row_mx[q] = mx; row_lse[q] = lse; }
        for (int v0 = tid; v0 < V; v0 += 256 * 8) {
            float z[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int v = v0 + 256 * u; z[u] = v < V ? lp[v] : 0.f; }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int v = v0 + 256 * u;
                if (v >= V || v == prev) continue;
                float cv = cum + ((z[u] * scale - mx) - lse);
                int ci = q * V + v;
                if (ortk_better(cv, ci, bv[MAXB - 1], bi[MAXB - 1])) {
#pragma unroll
                    for (int k = 0; k < MAXB; ++k) {
                        if (ortk_better(cv, ci, bv[k], bi[k])) {
                            const float tv = bv[k]; const int ti = bi[k];
                            bv[k] = cv; bi[k] = ci; cv = tv; ci = ti;
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < MAXB; ++k) { sv[tid * MAXB + k] = bv[k]; si[tid * MAXB + k] = bi[k]; }
    }
    __syncthreads();
    // b rounds of block-wide arg-max over the 256*MAXB staged candidates (each thread scans its own MAXB)
    for (int r = 0; r < b; ++r) {
        float mv = -INFINITY; int mi = 0x7FFFFFFF, mp = -1;
#pragma unroll
        for (int k = 0; k < MAXB; ++k) {
            const float v = sv[tid * MAXB + k]; const int i = si[tid * MAXB + k];
            if (ortk_better(v, i, mv, mi)) { mv = v; mi = i; mp = tid * MAXB + k; }
        }
        blk_argbest(mv, mi, mp, red_v, red_i, red_pos);
        if (tid == 0) {
            win_v[r] = mv; win_i[r] = mi;
            if (mp >= 0) sv[mp] = -INFINITY, si[mp] = 0x7FFFFFFF;
        }
        __syncthreads();
    }
    beam_commit(st, logp, t, scale, win_v, win_i, row_mx, row_lse, end_slot);
}

template <int NPT, bool FASTEXP = false, bool STATS = false>
__global__ __launch_bounds__(256) void beam_step_wide_kernel(BeamState st, const float* __restrict__ logp, int t, float scale) {
    __shared__ WideLds S;
    __shared__ int end_slot[WMAXB];
    const int b = st.b, L = st.L;
    const int nq = t == 0 ? 1 : b;
    const int cur = t & 1;
    const int64_t row0 = (int64_t)blockIdx.x * b;
    const int64_t srow0 = t == 0 ? (int64_t)blockIdx.x : row0;
    beam_select_wide<true, NPT, FASTEXP, STATS>(S, logp + srow0 * st.ldv, st.ldv, nq, b, st.V, scale, t == 0 ? nullptr : st.cum + row0,
                                                (st.decoding_constraint && t > 0) ? st.seq[cur] + row0 * L + t - 1 : nullptr, L,
                                                STATS ? st.gstats + srow0 * st.nblk * 2 : nullptr, st.nblk);
    beam_commit(st, logp, t, scale, S.win_v, S.win_i, S.row_mx, S.row_lse, end_slot);
}

// ortk_beam_select: the selection alone, winners to global memory
template <bool FUSED, int NPT>
__global__ __launch_bounds__(256) void beam_select_kernel(const float* __restrict__ logits, int64_t ld, const float* __restrict__ cum,
                                                          const int32_t* __restrict__ prev, int q, int b, int V, float scale,
                                                          float* __restrict__ val, int32_t* __restrict__ parent, int32_t* __restrict__ token) {
    __shared__ WideLds S;
    const int64_t row0 = (int64_t)blockIdx.x * q;
    beam_select_wide<FUSED, NPT, false, false>(S, logits + row0 * ld, ld, q, b, V, scale, cum + row0, prev ? prev + row0 : nullptr, 1, nullptr, 0);
    if ((int)threadIdx.x < b) {
        const int ix = S.win_i[threadIdx.x];
        const int64_t o = (int64_t)blockIdx.x * b + threadIdx.x;
        val[o] = S.win_v[threadIdx.x]; parent[o] = ix / V; token[o] = ix - (ix / V) * V;
    }
}

// ------------------------------------------------------------------------------------------------ grouped (diverse) beam step
// One local step t of ONE group of a diverse beam search (CaptionModel.batch_beam_search with group_size > 1, caption_model.py:33-52,
// 151-218): beam_step_wide_kernel's contract on the group's own BeamState (width b = beams per group), with every candidate's log-prob
// lowered by lambda x the number of beams of the image's EARLIER groups that hold the candidate's token at column t of their
// histories as they stand now.  Group p < g has then done min(t + g - p, L - 1) + 1 local steps (the schedule is staggered), so its
// current history is the ping-pong buffer of that parity.  The token log-prob stored by beam_commit is the unaugmented one; cum is
// the augmented sum.  g = 0: no penalty, the wide step's results bit for bit.
struct PenSrc {
    const int32_t* seq[2];    // group 0's ping-pong histories (BeamState.seq of group 0); group p's lie gstride elements further each
    int64_t gstride;
    int32_t g;                // index of this group = number of earlier groups; g * b <= ORTK_MAX_BEAM - 1
};
template <int NPT, bool FASTEXP = false, bool STATS = false>
__global__ __launch_bounds__(256) void beam_step_diverse_kernel(BeamState st, const float* __restrict__ logp, int t, float scale, PenSrc ps,
                                                                float lambda) {
    __shared__ WideLds S;
    __shared__ PenLds Pn;
    __shared__ int end_slot[WMAXB];
    const int b = st.b, L = st.L, tid = threadIdx.x;
    const int nq = t == 0 ? 1 : b;
    const int cur = t & 1;
    const int64_t row0 = (int64_t)blockIdx.x * b;
    const int64_t srow0 = t == 0 ? (int64_t)blockIdx.x : row0;
    const int n_pen = ps.g * b;
    int raw = -1;
    if (tid < n_pen) {
        const int p = tid / b, q = tid - p * b;
        const int steps = min(t + ps.g - p, L - 1) + 1;              // local steps group p has done
        raw = ((steps & 1) ? ps.seq[1] : ps.seq[0])[(int64_t)p * ps.gstride + (row0 + q) * L + t];
    }
    pen_build(Pn, raw, n_pen, lambda);
    beam_select_wide<true, NPT, FASTEXP, STATS, true>(S, logp + srow0 * st.ldv, st.ldv, nq, b, st.V, scale, t == 0 ? nullptr : st.cum + row0,
                                                      (st.decoding_constraint && t > 0) ? st.seq[cur] + row0 * L + t - 1 : nullptr, L,
                                                      STATS ? st.gstats + srow0 * st.nblk * 2 : nullptr, st.nblk, &Pn);
    beam_commit(st, logp, t, scale, S.win_v, S.win_i, S.row_mx, S.row_lse, end_slot);
}

// ortk_beam_select_diverse: the grouped selection alone, winners and their unaugmented log-probs to global memory
template <bool FUSED, int NPT>
__global__ __launch_bounds__(256) void beam_select_diverse_kernel(const float* __restrict__ logits, int64_t ld, const float* __restrict__ cum,
                                                                  const int32_t* __restrict__ prev, const int32_t* __restrict__ pen_tok, int n_pen,
                                                                  float lambda, int q, int b, int V, float scale, float* __restrict__ val,
                                                                  int32_t* __restrict__ parent, int32_t* __restrict__ token, float* __restrict__ tok_lp) {
    __shared__ WideLds S;
    __shared__ PenLds Pn;
    const int64_t row0 = (int64_t)blockIdx.x * q;
    pen_build(Pn, (int)threadIdx.x < n_pen ? pen_tok[(int64_t)blockIdx.x * n_pen + threadIdx.x] : -1, n_pen, lambda);
    beam_select_wide<FUSED, NPT, false, false, true>(S, logits + row0 * ld, ld, q, b, V, scale, cum + row0, prev ? prev + row0 : nullptr, 1, nullptr, 0, &Pn);
    if ((int)threadIdx.x < b) {
        const int ix = S.win_i[threadIdx.x];
        const int pr = ix / V, tk = ix - pr * V;
        const int64_t o = (int64_t)blockIdx.x * b + threadIdx.x;
        const float x = logits[(row0 + pr) * ld + tk];
        val[o] = S.win_v[threadIdx.x]; parent[o] = pr; token[o] = tk;
        tok_lp[o] = FUSED ? __fmaf_rn(x, scale, -S.row_mx[pr]) - S.row_lse[pr] : x;
    }
}

// stable top-b of each image's finished list by score (descending; earlier insertion wins ties)
__global__ __launch_bounds__(64) void beam_finalize_kernel(BeamState st, int64_t* __restrict__ seq_out, float* __restrict__ lp_out,
                                                           float* __restrict__ score_out) {
    __shared__ unsigned char taken[ORTK_MAX_BEAM * 64];
    const int img = blockIdx.x, lane = threadIdx.x;
    const int b = st.b, L = st.L, cap = b * L;
    const int cnt = st.done_cnt[img];
    for (int i = lane; i < cap; i += 64) taken[i] = 0;
    __syncthreads();
    for (int r = 0; r < b; ++r) {
        double best = -INFINITY; int bi = 0x7FFFFFFF;
        for (int i = lane; i < cnt; i += 64)
            if (!taken[i]) {
                const double p = st.done_p[(int64_t)img * cap + i];
                if (p > best || (p == best && i < bi)) { best = p; bi = i; }
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double op = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
            if (op > best || (op == best && oi < bi)) { best = op; bi = oi; }
        }
        const int64_t orow = (int64_t)img * b + r;
        if (bi != 0x7FFFFFFF) {
            const int64_t base = (int64_t)img * cap + bi;
            const int len = st.done_len[base];
            for (int u = lane; u < L; u += 64) {
                seq_out[orow * L + u] = u < len ? (int64_t)st.done_seq[base * L + u] : 0;
                lp_out[orow * L + u] = u < len ? st.done_lp[base * L + u] : 0.f;
            }
            if (lane == 0) { taken[bi] = 1; if (score_out) score_out[orow] = (float)best; }
        } else {
            for (int u = lane; u < L; u += 64) { seq_out[orow * L + u] = 0; lp_out[orow * L + u] = 0.f; }
            if (lane == 0 && score_out) score_out[orow] = 0.f;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ greedy / multinomial
__global__ void sample_init_kernel(SampleState st, int bos) {
    const int64_t n = (int64_t)st.rows * st.L;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) { st.seq[i] = 0; st.lp[i] = 0.f; }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < st.rows; i += (int64_t)gridDim.x * 256) {
        st.it[i] = bos; st.unfinished[i] = bos != st.eos;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { st.last_step[0] = -1; st.last_step[1] = -1; }
}

// what a row of the sampling state is at step t: the token it may not repeat (-1: none), whether it is one of the greedy rows of a
// combined call, whether its token is drawn, and the row the noise hash is keyed by
struct SampleRow { int prev; bool is_greedy, samp; int hrow; };
__device__ __forceinline__ SampleRow sample_row_id(const SampleState& st, int row, int t) {
    SampleRow r;
    r.prev = (st.decoding_constraint && t > 0) ? (int)st.seq[(int64_t)row * st.L + t - 1] : -1;
    r.is_greedy = st.greedy_stride > 0 && row % st.greedy_stride == 0;
    r.samp = st.sample && !r.is_greedy;
    // the hash is keyed by the row index the sample would have in a samples-only call
    const int64_t grow = st.row_offset + row;
    r.hrow = (int)(st.greedy_stride > 0 ? grow - grow / st.greedy_stride - 1 : grow);
    return r;
}

// the row's token of step t and its log-prob are known: the bookkeeping of every sampling step (one thread per row)
__device__ __forceinline__ void sample_commit(const SampleState& st, int row, int t, int tok, float lp, bool is_greedy) {
    const int unf = st.unfinished[row];
    st.it[row] = tok;
    st.seq[(int64_t)row * st.L + t] = unf ? tok : 0;     // seq[:, t] = it * unfinished   (transformer.py:546)
    st.lp[(int64_t)row * st.L + t] = lp;                 // NOT masked after EOS          (transformer.py:548)
    const int now = unf && (tok != st.eos);
    st.unfinished[row] = now;
    // the reference leaves the loop at the first step where no row is unfinished (transformer.py:550-551)
    int32_t* last = st.last_step + (is_greedy ? 1 : 0);
    if (unf && !now) atomicMax(last, t);
    if (now && t == st.L - 1) atomicMax(last, t);
}

__global__ __launch_bounds__(256) void sample_step_kernel(SampleState st, const float* __restrict__ logp, int t) {
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* lp = logp + (int64_t)row * st.ldv;
    const SampleRow id = sample_row_id(st, row, t);
    float mv = -INFINITY; int mi = 0x7FFFFFFF;
    for (int v = tid; v < st.V; v += 256) {
        if (v == id.prev) continue;
        float x = lp[v];
        if (id.samp) x = x / st.temperature + ortk_gumbel<false>(st.seed, t, id.hrow, v);
        if (ortk_better(x, v, mv, mi)) { mv = x; mi = v; }
    }
    blk_argbest(mv, mi, red_v, red_i);
    if (tid == 0) sample_commit(st, row, t, mi, lp[mi], id.is_greedy);
}

// A row of raw logits into registers (one read: z[u] is column tid + 256 u, 0 past V) and the statistics of its log-soft-max, max and
// lse = log sum exp(. - max), with the reductions of log_softmax_kernel in its element order
template <int NPT, bool FASTEXP>
__device__ __forceinline__ void row_lse(const float* __restrict__ lp, int V, float (&z)[NPT], float* sh_red, float& mx, float& lse) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int u = 0; u < NPT; ++u) { const int v = tid + 256 * u; z[u] = v < V ? lp[v] : 0.f; }
    float m = -INFINITY;
#pragma unroll
    for (int u = 0; u < NPT; ++u) if (tid + 256 * u < V) m = fmaxf(m, z[u]);
    mx = blk_max(m, sh_red);
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < NPT; ++u) if (tid + 256 * u < V) sum += exp_sel<FASTEXP>(z[u] - mx);
    sum = blk_sum(sum, sh_red);
    lse = logf(sum);
}

// Same step on RAW generator logits: the row stays in registers (one read), its log-soft-max statistics are taken with the
// reductions of log_softmax_kernel (bit-identical log-probabilities), then the arg-max / Gumbel-max runs on
// logp = (logit - max) - lse.  Saves the separate log-soft-max pass (read + write of rows x V fp32 per step).
template <int NPT, bool FASTEXP = false>
__global__ __launch_bounds__(256) void sample_step_fused_kernel(SampleState st, const float* __restrict__ logits, int t) {
    __shared__ float sh_red[4];
    __shared__ float red_v[4], red_l[4];
    __shared__ int red_i[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    float z[NPT], mx, lse;
    row_lse<NPT, FASTEXP>(logits + (int64_t)row * st.ldv, st.V, z, sh_red, mx, lse);
    const SampleRow id = sample_row_id(st, row, t);
    float mv = -INFINITY, ml = 0.f; int mi = 0x7FFFFFFF;
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
        const int v = tid + 256 * u;
        if (v >= st.V || v == id.prev) continue;
        const float l = (z[u] - mx) - lse;
        float x = l;
        if (id.samp) x = x / st.temperature + ortk_gumbel<FASTEXP>(st.seed, t, id.hrow, v);
        if (ortk_better(x, v, mv, mi)) { mv = x; mi = v; ml = l; }
    }
    blk_argbest(mv, mi, ml, red_v, red_i, red_l);
    if (tid == 0) sample_commit(st, row, t, mi, ml, id.is_greedy);
}

// ------------------------------------------------------------------------------------------------ truncated sampling (top-k / nucleus)
// The kept set of a row is a PREFIX of the total order of its candidates (larger logit first, lower column on equal logits; the banned
// column is no candidate): entry e is kept iff mu{entries strictly better than e} < lambda, with mu = count and lambda = min(top_k,
// candidates) for top-k, mu = soft-max(z / temperature) mass and lambda = top_p for the nucleus (caption_model.py:252-257).  mu is an
// integer count or an fp32 sum taken in ONE fixed order whatever the set (thread-sequential over the 40 registers with the entries
// outside the set as +0, xor tree over the wave, the four waves in order), so it is monotone along the order — fl(a + b) is monotone in
// both arguments — and two runs give the same bits.  The cut is found without a sort: a bit-wise descent over the order-preserving
// uint32 image of the logit (32 block-wide measures: the largest key T with mu{key >= T} >= lambda), then, only where several
// candidates share that logit, 14 more over the column.  No atomics, no global scratch.
struct TruncCut { uint32_t key; int col; int kept; float mass; };       // last kept entry (key, col); entries kept; their mass

// order-preserving image of a float (-0 counts as +0, as in the float compare)
__device__ __forceinline__ uint32_t trunc_key(float x) {
    const uint32_t b = __float_as_uint(x + 0.f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float trunc_unkey(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
__device__ __forceinline__ bool trunc_in(uint32_t key, int v, const TruncCut& c) { return key > c.key || (key == c.key && v <= c.col); }

// block-wide reduction that leaves the result in every thread; the two halves of `sh` alternate (`ph`), so one barrier per call is
// enough: the half call n writes was last read by call n - 2, which every thread has left before it passes the barrier of call n - 1
template <typename T, typename F>
__device__ __forceinline__ T blk_all(T v, F f, uint32_t* sh, int& ph) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = f(v, __shfl_xor(v, o, 64));
    uint32_t* b = sh + ((ph++ & 1) << 2);
    if ((threadIdx.x & 63) == 0) b[threadIdx.x >> 6] = __builtin_bit_cast(uint32_t, v);
    __syncthreads();
    T r = __builtin_bit_cast(T, b[0]);
    for (int w = 1; w < 4; ++w) r = f(r, __builtin_bit_cast(T, b[w]));
    return r;
}

// key[] (out): trunc_key of every entry.  A column that is no candidate (past V, or banned) counts as a logit of -inf: below every
// finite logit in the key order, and of weight exp(-inf) = 0.  w: the soft-max(z / temperature) weights of the candidates (the
// nucleus measures them; top-k forms them for kept_mass alone: 40 exponentials beside a descent of 32 rounds).  Block-uniform result.
template <int NPT, bool FASTEXP>
__device__ __forceinline__ TruncCut trunc_select(const float (&z)[NPT], uint32_t (&key)[NPT], int V, int prev, float temperature, int top_k,
                                                 float top_p, uint32_t* sh, int& ph) {
    const int tid = threadIdx.x;
    const auto iadd = [](int a, int b) { return a + b; };
    const auto fadd = [](float a, float b) { return a + b; };
    const auto imax = [](int a, int b) { return a > b ? a : b; };
    const auto umin = [](uint32_t a, uint32_t b) { return a < b ? a : b; };
    constexpr uint32_t KEY_NONE = 0x007FFFFFu;          // trunc_key(-inf)
    float w[NPT];
    int nc = 0;
    float m = -INFINITY;
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
        const int v = tid + 256 * u;
        const bool cand = v < V && v != prev;
        w[u] = cand ? z[u] : -INFINITY;
        key[u] = trunc_key(w[u]);
        nc += cand ? 1 : 0;
        m = fmaxf(m, w[u]);
    }
    const int ncand = blk_all(nc, iadd, sh, ph);
    TruncCut cut{0xFFFFFFFFu, -1, 0, 0.f};
    if (ncand == 0) return cut;
    const float mxc = blk_all(m, [](float a, float b) { return fmaxf(a, b); }, sh, ph);
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < NPT; ++u) { w[u] = exp_sel<FASTEXP>((w[u] - mxc) / temperature); s += w[u]; }
    const float tot = blk_all(s, fadd, sh, ph);
#pragma unroll
    for (int u = 0; u < NPT; ++u) w[u] = w[u] / tot;
    const bool by_count = top_k > 0;
    const int kk = top_k < ncand ? top_k : ncand;
    // mu{pred} < lambda
    const auto below = [&](auto pred) -> bool {
        if (by_count) {
            int c = 0;
#pragma unroll
            for (int u = 0; u < NPT; ++u) c += pred(u) ? 1 : 0;
            return blk_all(c, iadd, sh, ph) < kk;
        }
        float a = 0.f;
#pragma unroll
        for (int u = 0; u < NPT; ++u) a += pred(u) ? w[u] : 0.f;
        return blk_all(a, fadd, sh, ph) < top_p;
    };
    // (top-k: the kk best candidates have finite keys, so T ends above KEY_NONE and no trial at or below it is ever accepted)
    uint32_t T = 0;
    for (int b = 31; b >= 0; --b) {
        const uint32_t trial = T | (1u << b);
        if (!below([&](int u) { return key[u] >= trial; })) T = trial;
    }
    int C = 256 * NPT - 1;
    if (T == 0) {
        // not even the whole row reaches top_p (fp32 rounding of a total of 1): everything is kept
        uint32_t k = 0xFFFFFFFFu;
#pragma unroll
        for (int u = 0; u < NPT; ++u) if (key[u] > KEY_NONE) k = umin(k, key[u]);
        T = blk_all(k, umin, sh, ph);
    } else {
        int c = 0;
#pragma unroll
        for (int u = 0; u < NPT; ++u) c += key[u] == T;
        if (blk_all(c, iadd, sh, ph) > 1) {
            // several candidates carry the cut's logit: the largest column C whose entry still has mu{strictly better} < lambda.
            // tc: the column of an entry at the cut's logit; -1 for a better entry (before every column), past the row for a worse one
            int tc[NPT];
#pragma unroll
            for (int u = 0; u < NPT; ++u) tc[u] = key[u] == T ? tid + 256 * u : key[u] > T ? -1 : 256 * NPT;
            C = 0;
            for (int b = 13; b >= 0; --b) {
                const int trial = C | (1 << b);
                if (below([&](int u) { return tc[u] < trial; })) C = trial;
            }
        }
    }
    int lc = -1, kept = 0; float km = 0.f;
#pragma unroll
    for (int u = 0; u < NPT; ++u) if (key[u] == T && tid + 256 * u <= C) lc = tid + 256 * u;      // (columns ascend with u)
    cut.key = T; cut.col = blk_all(lc, imax, sh, ph);
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
        const bool in = trunc_in(key[u], tid + 256 * u, cut);
        kept += in ? 1 : 0;
        km += in ? w[u] : 0.f;
    }
    cut.kept = blk_all(kept, iadd, sh, ph);
    cut.mass = blk_all(km, fadd, sh, ph);
    return cut;
}

// sample_step_fused_kernel with the draw restricted to the kept set of the row: same statistics (the stored log-prob is that of the
// FULL distribution at temperature 1), same hash row, same bookkeeping; with top_k >= V bit-identical to it.  The noise is evaluated
// for the kept entries only.  Greedy rows (with_greedy) take the plain arg-max.
template <int NPT, bool FASTEXP = false>
__global__ __launch_bounds__(256) void sample_step_trunc_kernel(SampleState st, const float* __restrict__ logits, int t, int top_k, float top_p) {
    __shared__ float sh_red[4];
    __shared__ float red_v[4], red_l[4];
    __shared__ int red_i[4];
    __shared__ uint32_t sh_sel[8];
    const int row = blockIdx.x, tid = threadIdx.x;
    float z[NPT], mx, lse;
    row_lse<NPT, FASTEXP>(logits + (int64_t)row * st.ldv, st.V, z, sh_red, mx, lse);
    const SampleRow id = sample_row_id(st, row, t);
    uint32_t key[NPT];
    TruncCut cut{1u, 256 * NPT, 0, 0.f};        // every candidate (greedy rows)
    int ph = 0;
    if (id.samp) cut = trunc_select<NPT, FASTEXP>(z, key, st.V, id.prev, st.temperature, top_k, top_p, sh_sel, ph);
    float mv = -INFINITY, ml = 0.f; int mi = 0x7FFFFFFF;
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
        const int v = tid + 256 * u;
        if (v >= st.V || v == id.prev) continue;
        if (id.samp && !trunc_in(key[u], v, cut)) continue;
        const float l = (z[u] - mx) - lse;
        float x = l;
        if (id.samp) x = x / st.temperature + ortk_gumbel<FASTEXP>(st.seed, t, id.hrow, v);
        if (ortk_better(x, v, mv, mi)) { mv = x; mi = v; ml = l; }
    }
    blk_argbest(mv, mi, ml, red_v, red_i, red_l);
    if (tid == 0) sample_commit(st, row, t, mi, ml, id.is_greedy);
}

// ortk_sample_truncate: the cut of every row, by the device function of the step kernel
template <int NPT, bool FASTEXP>
__global__ __launch_bounds__(256) void sample_truncate_kernel(const float* __restrict__ logits, int V, int64_t ld, float temperature, int top_k, float top_p,
                                                              const int64_t* __restrict__ banned, int32_t* __restrict__ kept, float* __restrict__ thr,
                                                              int32_t* __restrict__ thr_col, float* __restrict__ kept_mass) {
    __shared__ uint32_t sh_sel[8];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* lp = logits + (int64_t)row * ld;
    float z[NPT];
#pragma unroll
    for (int u = 0; u < NPT; ++u) { const int v = tid + 256 * u; z[u] = v < V ? lp[v] : 0.f; }
    const int prev = banned ? (int)banned[row] : -1;
    uint32_t key[NPT];
    int ph = 0;
    const TruncCut cut = trunc_select<NPT, FASTEXP>(z, key, V, prev, temperature, top_k, top_p, sh_sel, ph);
    if (tid == 0) {
        kept[row] = cut.kept; thr[row] = cut.kept ? trunc_unkey(cut.key) : -INFINITY; thr_col[row] = cut.col; kept_mass[row] = cut.mass;
    }
}

// The sampling step on the generator's own epilogue output (ortk_gemm_args.tile_samp + tile_stats): per row and block of 64 logits the
// best Gumbel-max candidate {key, column, logit} and the soft-max partials {max, sum exp}.  One wave per row: arg-max over the blocks
// (same total order as the row kernels: larger key, lower column on a tie), log-sum-exp from the partials, log-prob of the chosen token,
// then sample_commit.  The logit rows (62 MB per position of the SCST rollout) are neither written nor read.
template <bool FASTEXP>
__global__ __launch_bounds__(256) void sample_combine_kernel(SampleState st, const float* __restrict__ gstats, const float* __restrict__ gsamp, int nblk, int t) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= st.rows) return;
    const float* gs = gstats + (int64_t)row * nblk * 2;
    const float* gp = gsamp + (int64_t)row * nblk * 4;
    float m = -INFINITY, mv = -INFINITY, mz = 0.f; int mi = 0x7FFFFFFF;
    for (int b = lane; b < nblk; b += 64) {
        m = fmaxf(m, gs[2 * b]);
        const float x = gp[4 * b]; const int i = __float_as_int(gp[4 * b + 1]);
        if (ortk_better(x, i, mv, mi)) { mv = x; mi = i; mz = gp[4 * b + 2]; }
    }
    m = wave_max(m);
    float sum = 0.f;
    for (int b = lane; b < nblk; b += 64) { const float sb = gs[2 * b + 1]; if (sb > 0.f) sum += sb * exp_sel<FASTEXP>(gs[2 * b] - m); }
    sum = wave_sum(sum);
    wave_argbest(mv, mi, mz);
    if (lane == 0) sample_commit(st, row, t, mi, (mz - m) - logf(sum), st.greedy_stride > 0 && row % st.greedy_stride == 0);
}

__global__ void sample_finalize_kernel(SampleState st) {
    const int64_t n = (int64_t)st.rows * st.L;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int t = (int)(i % st.L);
        const int64_t row = i / st.L;
        const int last = st.last_step[(st.greedy_stride > 0 && row % st.greedy_stride == 0) ? 1 : 0];
        if (t > last) { st.lp[i] = 0.f; st.seq[i] = 0; }
    }
}

inline unsigned ew_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ortk_cdiv(n, 256), 2048)); }

}  // namespace

int kv_append(const float* qkv, void* ck, void* cv, int32_t kvdt, int64_t rows, int32_t d, int32_t row_mult, int32_t tmax, int32_t t,
              hipStream_t s) {
    if (rows == 0) return 0;
    hipLaunchKernelGGL(kv_append_kernel, dim3(ew_grid(rows * d)), dim3(256), 0, s, qkv, ck, cv, (int)kvdt, rows, d, row_mult, tmax, t);
    ORTK_CHECK_LAUNCH();
    return 0;
}
int decode_poison(const int32_t* status, int64_t* seq, float* lp, float* score, int64_t nseq, int64_t nscore, hipStream_t s) {
    hipLaunchKernelGGL(decode_poison_kernel, dim3(64), dim3(256), 0, s, status, seq, lp, score, nseq, nscore);
    ORTK_CHECK_LAUNCH();
    return 0;
}
int fill_i64(int64_t* p, int64_t n, int64_t v, hipStream_t s) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(fill_i64_kernel, dim3(ew_grid(n)), dim3(256), 0, s, p, n, v);
    ORTK_CHECK_LAUNCH();
    return 0;
}
int fill_i32(int32_t* p, int64_t n, int32_t v, hipStream_t s) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(fill_i32_kernel, dim3(ew_grid(n)), dim3(256), 0, s, p, n, v);
    ORTK_CHECK_LAUNCH();
    return 0;
}
int kvidx_init(int32_t* kvidx, int64_t rows, int32_t row_mult, int32_t tmax, hipStream_t s) {
    if (rows == 0) return 0;
    hipLaunchKernelGGL(kvidx_init_kernel, dim3(ew_grid(rows)), dim3(256), 0, s, kvidx, rows, row_mult, tmax);
    ORTK_CHECK_LAUNCH();
    return 0;
}
int beam_step(const BeamState& st, const float* logp, int32_t t, hipStream_t s, float scale, bool fast_exp, bool wide) {
    if (st.b < 1 || st.b > ORTK_MAX_BEAM) return ORTK_EINVAL;
    if (st.B == 0) return 0;
    // the instance <NPT, FASTEXP, STATS> of either step kernel: the same mode picks the same instance of both
    const bool stats = fast_exp && st.gstats && scale == 1.f && st.nblk <= 256 && st.nblk * 64 >= st.V, reg_rows = st.V <= 256 * 40;
#define ORTK_BEAM_STEP(kernel, ...) hipLaunchKernelGGL((kernel<__VA_ARGS__>), dim3((unsigned)st.B), dim3(256), 0, s, st, logp, t, scale)
#define ORTK_BEAM_STEP_PICK(kernel)                                   \
    if (stats) ORTK_BEAM_STEP(kernel, 0, true, true);                 \
    else if (reg_rows && fast_exp) ORTK_BEAM_STEP(kernel, 40, true);  \
    else if (reg_rows) ORTK_BEAM_STEP(kernel, 40);                    \
    else ORTK_BEAM_STEP(kernel, 0)
    if (wide || st.b > MAXB) { ORTK_BEAM_STEP_PICK(beam_step_wide_kernel); }      // 9 .. 32 beams (and the test switch)
    else { ORTK_BEAM_STEP_PICK(beam_step_kernel); }
#undef ORTK_BEAM_STEP_PICK
#undef ORTK_BEAM_STEP
    ORTK_CHECK_LAUNCH();
    return 0;
}
int beam_step_diverse(const BeamState& st, const float* logp, int32_t t, hipStream_t s, float scale, bool fast_exp, const int32_t* const seq0[2],
                      int64_t gstride, int32_t g, float lambda) {
    if (st.b < 1 || st.b > ORTK_MAX_BEAM || g < 0 || (int64_t)g * st.b > ORTK_MAX_BEAM - 1 || !(lambda >= 0.f) || lambda == INFINITY) return ORTK_EINVAL;
    if (st.B == 0) return 0;
    PenSrc ps; ps.seq[0] = seq0[0]; ps.seq[1] = seq0[1]; ps.gstride = gstride; ps.g = g;
    // the instance <NPT, FASTEXP, STATS> beam_step picks in the same mode
    const bool stats = fast_exp && st.gstats && scale == 1.f && st.nblk <= 256 && st.nblk * 64 >= st.V, reg_rows = st.V <= 256 * 40;
#define ORTK_BEAM_STEP(...) hipLaunchKernelGGL((beam_step_diverse_kernel<__VA_ARGS__>), dim3((unsigned)st.B), dim3(256), 0, s, st, logp, t, scale, ps, lambda)
    if (stats) ORTK_BEAM_STEP(0, true, true);
    else if (reg_rows && fast_exp) ORTK_BEAM_STEP(40, true);
    else if (reg_rows) ORTK_BEAM_STEP(40);
    else ORTK_BEAM_STEP(0);
#undef ORTK_BEAM_STEP
    ORTK_CHECK_LAUNCH();
    return 0;
}
int beam_finalize(const BeamState& st, int64_t* seq_out, float* lp_out, float* score_out, hipStream_t s) {
    if (st.b < 1 || st.b > ORTK_MAX_BEAM || st.b * st.L > ORTK_MAX_BEAM * 64) return ORTK_EINVAL;
    if (st.B == 0) return 0;
    hipLaunchKernelGGL(beam_finalize_kernel, dim3((unsigned)st.B), dim3(64), 0, s, st, seq_out, lp_out, score_out);
    ORTK_CHECK_LAUNCH();
    return 0;
}
int sample_init(const SampleState& st, int32_t bos, hipStream_t s) {
    hipLaunchKernelGGL(sample_init_kernel, dim3(ew_grid((int64_t)st.rows * st.L)), dim3(256), 0, s, st, bos);
    ORTK_CHECK_LAUNCH();
    return 0;
}
int sample_step(const SampleState& st, const float* logp, int32_t t, hipStream_t s, bool fused, bool fast_exp) {
    if (st.rows == 0) return 0;
    if (fused) {       // `logp` holds raw logits (V <= 10 240: the caller checks sample_step_can_fuse)
        if (st.V > 256 * 40) return ORTK_EINVAL;
        if (fast_exp) hipLaunchKernelGGL((sample_step_fused_kernel<40, true>), dim3((unsigned)st.rows), dim3(256), 0, s, st, logp, t);
        else hipLaunchKernelGGL(sample_step_fused_kernel<40>, dim3((unsigned)st.rows), dim3(256), 0, s, st, logp, t);
        ORTK_CHECK_LAUNCH();
        return 0;
    }
    hipLaunchKernelGGL(sample_step_kernel, dim3((unsigned)st.rows), dim3(256), 0, s, st, logp, t);
    ORTK_CHECK_LAUNCH();
    return 0;
}
int sample_step_trunc(const SampleState& st, const float* logits, int32_t t, hipStream_t s, bool fast_exp, int32_t top_k, float top_p) {
    if (st.V > 256 * 40 || (top_k > 0) == (top_p > 0.f) || top_k < 0 || !(top_p >= 0.f && top_p < 1.f)) return ORTK_EINVAL;
    if (st.rows == 0) return 0;
    if (fast_exp) hipLaunchKernelGGL((sample_step_trunc_kernel<40, true>), dim3((unsigned)st.rows), dim3(256), 0, s, st, logits, t, top_k, top_p);
    else hipLaunchKernelGGL(sample_step_trunc_kernel<40>, dim3((unsigned)st.rows), dim3(256), 0, s, st, logits, t, top_k, top_p);
    ORTK_CHECK_LAUNCH();
    return 0;
}
int sample_combine(const SampleState& st, const float* gstats, const float* gsamp, int32_t nblk, int32_t t, hipStream_t s, bool fast_exp) {
    if (st.rows == 0) return 0;
    const dim3 grid((unsigned)((st.rows + 3) / 4));
    if (fast_exp) hipLaunchKernelGGL(sample_combine_kernel<true>, grid, dim3(256), 0, s, st, gstats, gsamp, (int)nblk, (int)t);
    else hipLaunchKernelGGL(sample_combine_kernel<false>, grid, dim3(256), 0, s, st, gstats, gsamp, (int)nblk, (int)t);
    ORTK_CHECK_LAUNCH();
    return 0;
}
int sample_finalize(const SampleState& st, hipStream_t s) {
    if (st.rows == 0) return 0;
    hipLaunchKernelGGL(sample_finalize_kernel, dim3(ew_grid((int64_t)st.rows * st.L)), dim3(256), 0, s, st);
    ORTK_CHECK_LAUNCH();
    return 0;
}

}  // namespace ortk

extern "C" int ortk_sample_truncate(const float* logits, int64_t rows, int32_t V, int64_t ld, float temperature, int32_t top_k, float top_p,
                                    const int64_t* banned, int32_t fast_exp, int32_t* kept, float* thr, int32_t* thr_col, float* kept_mass,
                                    ortk_stream stream) {
    if (!logits || !kept || !thr || !thr_col || !kept_mass || rows < 0 || rows > 0x7FFFFFFF) return ORTK_EINVAL;
    if (V < 1 || V > 256 * 40 || ld < V || !(temperature > 0.f) || top_k < 0 || !(top_p >= 0.f && top_p < 1.f)) return ORTK_EINVAL;
    if ((top_k > 0) == (top_p > 0.f)) return ORTK_EINVAL;          // exactly one of the two
    if (rows == 0) return 0;
    hipStream_t s = ortk_s(stream);
    if (fast_exp) hipLaunchKernelGGL((ortk::sample_truncate_kernel<40, true>), dim3((unsigned)rows), dim3(256), 0, s, logits, (int)V, ld, temperature, (int)top_k, top_p, banned, kept, thr, thr_col, kept_mass);
    else hipLaunchKernelGGL((ortk::sample_truncate_kernel<40, false>), dim3((unsigned)rows), dim3(256), 0, s, logits, (int)V, ld, temperature, (int)top_k, top_p, banned, kept, thr, thr_col, kept_mass);
    ORTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int ortk_beam_select(const float* logits, int64_t ld, const float* cum, const int32_t* prev, int32_t B, int32_t q, int32_t b,
                                int32_t V, int32_t fused, float scale, float* val, int32_t* parent, int32_t* token, ortk_stream stream) {
    if (!logits || !cum || !val || !parent || !token || B < 0 || V < 1 || ld < V) return ORTK_EINVAL;
    if (b < 1 || b > ORTK_MAX_BEAM || (q != 1 && q != b) || (int64_t)b > (int64_t)q * V || (int64_t)q * V > 0x7FFFFFFF) return ORTK_EINVAL;
    if (B == 0) return 0;
    hipStream_t s = ortk_s(stream);
    const dim3 grid((unsigned)B);
    if (!fused) hipLaunchKernelGGL((ortk::beam_select_kernel<false, 0>), grid, dim3(256), 0, s, logits, ld, cum, prev, (int)q, (int)b, (int)V, 1.f, val, parent, token);
    else if (V <= 256 * 40) hipLaunchKernelGGL((ortk::beam_select_kernel<true, 40>), grid, dim3(256), 0, s, logits, ld, cum, prev, (int)q, (int)b, (int)V, scale, val, parent, token);
    else hipLaunchKernelGGL((ortk::beam_select_kernel<true, 0>), grid, dim3(256), 0, s, logits, ld, cum, prev, (int)q, (int)b, (int)V, scale, val, parent, token);
    ORTK_CHECK_LAUNCH();
    return 0;
}

extern "C" int ortk_beam_select_diverse(const float* logits, int64_t ld, const float* cum, const int32_t* prev, const int32_t* pen_tok,
                                        int32_t n_pen, float lambda, int32_t B, int32_t q, int32_t b, int32_t V, int32_t fused, float scale,
                                        float* val, int32_t* parent, int32_t* token, float* tok_lp, ortk_stream stream) {
    if (!logits || !cum || !val || !parent || !token || !tok_lp || B < 0 || V < 1 || ld < V) return ORTK_EINVAL;
    if (b < 1 || b > ORTK_MAX_BEAM || (q != 1 && q != b) || (int64_t)b > (int64_t)q * V || (int64_t)q * V > 0x7FFFFFFF) return ORTK_EINVAL;
    if (n_pen < 0 || n_pen > ORTK_MAX_BEAM - 1 || (n_pen > 0 && !pen_tok) || !(lambda >= 0.f) || lambda == INFINITY) return ORTK_EINVAL;
    if (B == 0) return 0;
    hipStream_t s = ortk_s(stream);
    const dim3 grid((unsigned)B);
#define ORTK_SELECT_DIVERSE(F, N, sc) hipLaunchKernelGGL((ortk::beam_select_diverse_kernel<F, N>), grid, dim3(256), 0, s, logits, ld, cum, prev, pen_tok, (int)n_pen, lambda, (int)q, (int)b, (int)V, sc, val, parent, token, tok_lp)
    if (!fused) ORTK_SELECT_DIVERSE(false, 0, 1.f);
    else if (V <= 256 * 40) ORTK_SELECT_DIVERSE(true, 40, scale);
    else ORTK_SELECT_DIVERSE(true, 0, scale);
#undef ORTK_SELECT_DIVERSE
    ORTK_CHECK_LAUNCH();
    return 0;
}
