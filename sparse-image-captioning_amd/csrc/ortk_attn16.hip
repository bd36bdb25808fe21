// ortk_attn16.hip — bf16-MFMA attention for the mixed-precision mode (ortk_attn_args.precision = 1), forward and backward,
// for the two block shapes of the training step: encoder self-attention (36 x 36 regions, additive geometry bias) and
// decoder cross-attention (all captions of an image, 5 x 17 = 85 query rows, against its 36 regions); dk = 64.
//
// Same mathematics as the fp32-MFMA kernels of ortk_attn.hip (transformer.py:285-295, relation_transformer.py:258-293)
// — score = q.k / sqrt(dk); score[mask == 0] = -1e9; score += bias; P = softmax; O = dropout(P) V — with the operands of
// the four small products rounded to bf16 (fp32 accumulation, fp32 soft-max, fp32 P saved for the backward).  Why a
// second family: the fp32 kernels keep fp32 images of Q, K, V, dO, dS, P in LDS (109 KB for the cross-attention backward:
// ONE workgroup per CU, its load -> compute -> store phases fully exposed, 166 us where the HBM traffic needs 40) and
// feed v_mfma_f32_16x16x4_f32 one dword per lane and multiply-add.  Here every image is bf16 with 144-byte rows (30 KB
// forward, 53-71 KB backward: 2-5 workgroups per CU), a fragment is one ds_read_b128 or two ds_read_b64_tr_b16, and a
// 16 x 16 x 64 product is two v_mfma_f32_16x16x32_bf16.
//
// Layout rules (lane = (lr = lane & 15, lq = lane >> 4); MFMA(X, Y) gives D[x = 4*lq + r][y = lr], both operands
// supplying [index = lr][k = 8*lq .. 8*lq + 7]):
//   * every product is computed TRANSPOSED so that a lane ends up with 4 CONSECUTIVE elements of an output row:
//     scores S^T[key j = 16*jt + 4*lq + r][query i = lr] (soft-max over keys = in-lane + 2 shuffles; P rows, bias rows and
//     the LDS images of P / dS are 16- and 8-byte vector accesses), outputs O / dQ / dK / dV as [feature 4 consecutive][row];
//   * an operand whose k index runs along its image ROWS (K in dS.K, Q / dO / dS / P in the dK, dV products, V in P.V) is
//     gathered by the hardware-transposing LDS read; padded k ranges (keys 36 -> 64, queries 85 -> 96, 36 -> 64) are zero
//     rows / columns of the images.
// The pitch of 72 bf16 (144 B) makes the 16 rows of a ds_read_b128 service group fall on 16 distinct 16-byte slots.
//
// Three mappings of ONE per-tile code (fwd16_tile, bwd16_tile1, bwd16_tile2; bit-identical results), forward and backward:
//   * attn16_*_kernel, the wave-per-tile kernels: a workgroup per (group, head), a wave per 16-row query tile, K / V / Q / dO
//     through LDS images (stage_rows).  Every served shape, and the only mapping for fp32 inputs.
//   * attn16b_*_kernel, the block kernels (ortk_tuning.attn16_block): bf16 inputs, at most 64 keys and 96 query rows.  Three
//     waves whatever Lq, up to two query tiles per wave, half the LDS per workgroup and so more workgroups per compute unit.
//   * attn16s_*_kernel, the short kernels (ortk_tuning.attn16_short): bf16 inputs, at most 32 query rows and 32 keys (the
//     decoder's causal self-attention).  A WAVE per (group, head), no workgroup barrier.
// What the six kernels share besides the tile code: the ragged-group geometry (group_geo), the per-tile row setup (tile_rows),
// the register stager of the block and short kernels (stage_ld / stage_st), the row-fragment loads (ld_row_frags), the image
// clear (zero_cols), and one LDS layout per kernel (*Lds) that gives the kernel its pointers and attn16_plan its byte count.
// Two exceptions, both for registers (profiles/attention_refactor.txt): attn16b_bwd_kernel spells its prologue out, and so do the
// instances of attn16b_fwd_kernel that run two query tiles per wave.
#include <cstdlib>
#include <type_traits>
#include "ortk_internal.h"

namespace {

constexpr int P16 = 72;                 // bf16 elements per row of an image with up to 64 columns (keys, or the 64 features of a head)

__device__ __forceinline__ void wsync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

// Key-indexed geometry for njt key tiles (Lk <= 16 * njt <= 128): KJ = key range as a k dimension (multiple of 32, zero-
// padded), PJ = pitch of the [query][key] images (KJ + 8: the same 16-distinct-slots property as P16 for its row length).
__host__ __device__ constexpr int key_kj(int njt) { return njt <= 2 ? 32 : njt <= 4 ? 64 : njt <= 6 ? 96 : 128; }
__host__ __device__ constexpr int key_pj(int njt) { return njt <= 4 ? P16 : 136; }
template <int NJT> struct KeyGeo { static constexpr int KJ = key_kj(NJT), PJ = key_pj(NJT); };
constexpr int KJS = 32, PJS = KJS + 8;            // key range and [query][key] image pitch of the short kernels
constexpr int NWB = 3, NTB = 64 * NWB;            // waves / threads per workgroup of the block (attn16b) kernels

// The LDS layout of each kernel, declared once: the offsets (bf16 elements into sm16[]) its images start at, and the dynamic-LDS
// bytes its launch asks for.  (dk = features per head, image pitch dk + 8; nw = waves; Lqp = query rows padded to 32.)
__host__ __device__ constexpr int imax(int a, int b) { return a > b ? a : b; }
struct Fwd16Lds {      // attn16_fwd_kernel: K [16 njt][PD], V [KJ][PD], a P image [16][PJ] per wave, the key mask [128] floats
    int V, P, mask, end;
    __host__ __device__ constexpr Fwd16Lds(int njt, int dk, int nw)
        : V(16 * njt * (dk + 8)), P(V + key_kj(njt) * (dk + 8)), mask(P + 16 * nw * key_pj(njt)), end(mask + 2 * 128) {}
};
struct Fwd16sLds {     // attn16s_fwd_kernel, per wave: V [KJS][PD], P [16][PJS], the key mask [32] floats
    int P, mask, end;
    __host__ __device__ constexpr Fwd16sLds(int dk) : P(KJS * (dk + 8)), mask(P + 16 * PJS), end(mask + 2 * 32) {}
};
struct Fwd16bLds {     // attn16b_fwd_kernel: V [KJ][PD], then K [16 njt][PD] whose bytes become the NWB P images [16][PJ], the key mask [64] floats
    int K, mask, end;
    __host__ __device__ constexpr Fwd16bLds(int njt, int dk)
        : K(key_kj(njt) * (dk + 8)), mask(K + imax(16 * njt * (dk + 8), NWB * 16 * key_pj(njt))), end(mask + 2 * 64) {}
};
struct Bwd16Lds {      // attn16_bwd_kernel: K [KJ][PD], V [16 njt][PD], Q and dO [Lqp][PD], dS and dropped P [Lqp][PJ]
    int V, Q, G, S, D, end;
    __host__ __device__ constexpr Bwd16Lds(int njt, int dk, int Lqp)
        : V(key_kj(njt) * (dk + 8)), Q(V + 16 * njt * (dk + 8)), G(Q + Lqp * (dk + 8)), S(G + Lqp * (dk + 8)), D(S + Lqp * key_pj(njt)), end(D + Lqp * key_pj(njt)) {}
};
struct Bwd16sLds {     // attn16s_bwd_kernel, per wave: X [32][PD] (K, then Q, then dO), dS and dropped P [32][PJS]
    int S, D, end;
    __host__ __device__ constexpr Bwd16sLds(int dk) : S(32 * (dk + 8)), D(S + 32 * PJS), end(D + 32 * PJS) {}
};
struct Bwd16bLds {     // attn16b_bwd_kernel: X [max(KJ, Lqp)][PD] (K, then Q, then dO), dS and dropped P [Lqp][PJ]
    int S, D, end;
    __host__ __device__ constexpr Bwd16bLds(int njt, int dk, int Lqp)
        : S(imax(key_kj(njt), Lqp) * (dk + 8)), D(S + Lqp * key_pj(njt)), end(D + Lqp * key_pj(njt)) {}
};
template <typename L> constexpr size_t lds_bytes(const L& l) { return (size_t)l.end * sizeof(__bf16); }

// [index = row][k = k0 .. k0+7]: 8 consecutive elements of an image row
template <int PITCH = P16>
__device__ __forceinline__ bf16x8 frag_row(const __bf16* img, int row, int k0) {
    return *reinterpret_cast<const bf16x8*>(img + row * PITCH + k0);
}
// [index = x0 + lr][k = k0 + 8*lq .. +7] where k runs along the image ROWS: two transposing reads of 4 rows x 16 columns
template <int PITCH = P16>
__device__ __forceinline__ bf16x8 frag_tr(const __bf16* img, int k0, int x0, int lane) {
    const int lr = lane & 15, lq = lane >> 4;
    const __bf16* p = img + (k0 + 8 * lq + (lr >> 2)) * PITCH + x0 + 4 * (lane & 3);
    typedef bf16x4 __attribute__((address_space(3))) * lds4;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4)(p));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4)(p + 4 * PITCH));
    return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
__device__ __forceinline__ bf16x4 cvt4(float4 v) { return (bf16x4){(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w}; }
__device__ __forceinline__ bf16x8 cvt8(float4 a, float4 b) {
    return (bf16x8){(__bf16)a.x, (__bf16)a.y, (__bf16)a.z, (__bf16)a.w, (__bf16)b.x, (__bf16)b.y, (__bf16)b.z, (__bf16)b.w};
}
__device__ __forceinline__ f32x4 mma(bf16x8 x, bf16x8 y, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, y, acc, 0, 0, 0); }

// rows [0, rows) of a (.., 64)-column matrix slice (fp32 or bf16 in memory) -> bf16 image; rows [rows, rows_pad) are zeroed
// (DKT = features per head: 64 or 32; image pitch DKT + 8)
template <int DKT>
__device__ __forceinline__ void stage_rows(__bf16* img, const float* src, int64_t ld, int rows, int rows_pad, int tid, int nthr) {
    constexpr int CPR = DKT / 4;
    for (int idx = tid; idx < rows_pad * CPR; idx += nthr) {
        const int r = idx / CPR, c = (idx % CPR) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < rows) v = *reinterpret_cast<const float4*>(src + (int64_t)r * ld + c);
        *reinterpret_cast<bf16x4*>(img + r * (DKT + 8) + c) = cvt4(v);
    }
}
template <int DKT>
__device__ __forceinline__ void stage_rows(__bf16* img, const __bf16* src, int64_t ld, int rows, int rows_pad, int tid, int nthr) {
    constexpr int CPR = DKT / 8;
    for (int idx = tid; idx < rows_pad * CPR; idx += nthr) {
        const int r = idx / CPR, c = (idx % CPR) * 8;
        bf16x8 v = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        if (r < rows) v = *reinterpret_cast<const bf16x8*>(src + (int64_t)r * ld + c);
        *reinterpret_cast<bf16x8*>(img + r * (DKT + 8) + c) = v;
    }
}
// 8 consecutive elements of a global row as an MFMA fragment
__device__ __forceinline__ bf16x8 ld_frag(const float* p) { return cvt8(*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4)); }
__device__ __forceinline__ bf16x8 ld_frag(const __bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }

// Where the row fragments [index = 16*jt + lr][k = 32*ks + 8*lq ..] of a key-indexed operand come from (K in the score product,
// V in dP^T = V dO^T): an LDS image (the block kernels) or registers loaded straight from global memory (the short kernels).
template <int PD> struct LdsRowFrags {
    const __bf16* img; int lr, lq;
    __device__ __forceinline__ bf16x8 operator()(int jt, int ks) const { return frag_row<PD>(img, 16 * jt + lr, 32 * ks + 8 * lq); }
};
template <int NJT, int NKS> struct RegRowFrags {
    bf16x8 f[NJT][NKS];
    __device__ __forceinline__ bf16x8 operator()(int jt, int ks) const { return f[jt][ks]; }
};
// Element (r, c) of a matrix slice behind a uniform base.  OFF32 (the block kernels): a 32-bit offset per lane, so that a load
// holds one address register and not two (their register budget: attn16b_fwd_kernel); otherwise 64-bit.
template <bool OFF32> __device__ __forceinline__ int64_t row_off(int r, int64_t ld, int c) {
    if constexpr (OFF32) return (unsigned)r * (unsigned)ld + (unsigned)c;
    else return (int64_t)r * ld + c;
}
// rows [0, rows) of the group's rows, head h, as such fragments; rows past the count are zero (what stage_rows leaves in an image)
template <bool OFF32, int NJT, int NKS>
__device__ __forceinline__ void ld_row_frags(RegRowFrags<NJT, NKS>& out, const __bf16* src, int64_t ld, int rows, int lane) {
    const int lr = lane & 15, lq = lane >> 4;
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            out.f[jt][ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
            if (16 * jt + lr < rows) out.f[jt][ks] = ld_frag(src + row_off<OFF32>(16 * jt + lr, ld, 32 * ks + 8 * lq));
        }
}
// One row of a [..][Lk] fp32 tensor (bias, saved P) as this lane's 4 consecutive keys of every key tile; zero where `on` is
// false or the key does not exist
template <int NJT>
__device__ __forceinline__ void ld_keys4(float4 (&out)[NJT], const float* base, bool on, int64_t prow, int Lk, int lq) {
    const bool vec_p = (Lk & 3) == 0;               // rows start 16-byte aligned
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt) {
        const int j0 = 16 * jt + 4 * lq;
        out[jt] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on) {
            if (vec_p && j0 < Lk) out[jt] = *reinterpret_cast<const float4*>(base + prow + j0);
            else { float* q = &out[jt].x; for (int r = 0; r < 4; ++r) if (j0 + r < Lk) q[r] = base[prow + j0 + r]; }
        }
    }
}
// The register stager of the short kernels (NT = 64: one wave, ROWS = 32) and of the block kernels (NT = NTB): thread tid's share
// of a ROWS-row image.  stage_ld: rows [0, rows) of a bf16 matrix slice into registers, zero past the count; stage_st: rows
// [0, rows_st) into the image (pitch DKT + 8).  Split in two so that the loads are issued with every other load of the workgroup.
template <int DKT, int ROWS, int NT> struct Stage { static constexpr int N = (ROWS * (DKT / 8) + NT - 1) / NT; };      // 16-byte pieces per thread
template <int DKT, int ROWS, int NT, int N = Stage<DKT, ROWS, NT>::N>
__device__ __forceinline__ void stage_ld(bf16x8 (&v)[N], const __bf16* src, int64_t ld, int rows, int tid) {
    constexpr int CPR = DKT / 8;
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const int idx = tid + NT * n, r = idx / CPR, c = (idx % CPR) * 8;
        v[n] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        if (r < rows) v[n] = *reinterpret_cast<const bf16x8*>(src + row_off<NT != 64>(r, ld, c));
    }
}
template <int DKT, int ROWS, int NT, int N = Stage<DKT, ROWS, NT>::N>
__device__ __forceinline__ void stage_st(__bf16* img, const bf16x8 (&v)[N], int rows_st, int tid) {
    constexpr int CPR = DKT / 8;
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const int idx = tid + NT * n, r = idx / CPR, c = (idx % CPR) * 8;
        if (r < rows_st) *reinterpret_cast<bf16x8*>(img + r * (DKT + 8) + c) = v[n];
    }
}
// Columns [0, COLS) of `rows` rows of a [query][key] image (pitch PJ) to zero: the key columns 16 * NJT .. KJ - 1, and the rows of a
// tile that is not run, are never written by a tile.  COLS = PJ: the image is contiguous (16-byte stores, the padding included).
template <int PJ, int COLS>
__device__ __forceinline__ void zero_cols(__bf16* img, int rows, int tid, int nthr) {
    constexpr int VN = COLS == PJ ? 8 : 4, CPR = COLS / VN;
    for (int idx = tid; idx < rows * CPR; idx += nthr) {
        __bf16* p = COLS == PJ ? img + idx * VN : img + (idx / CPR) * PJ + (idx % CPR) * VN;
        if constexpr (VN == 8) *reinterpret_cast<bf16x8*>(p) = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        else *reinterpret_cast<bf16x4*>(p) = cvt4(make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

// Ragged groups (ortk_attn_args.q_off): group g's first query row and its row count; with kv_ragged its keys are those rows.
struct GroupGeo { int64_t qrow0; int Lqg; int64_t krow0; int Lkg; };
__device__ __forceinline__ GroupGeo group_geo(const ortk_attn_args& a, int g) {
    int64_t qrow0 = (int64_t)g * a.Lq;
    int Lqg = a.Lq;
    if (a.q_off) {                                  // both entries in one round trip
        const int o0 = a.q_off[(int64_t)g * a.q_off_stride], o1 = a.q_off[(int64_t)(g + 1) * a.q_off_stride];
        qrow0 = o0; Lqg = min(a.Lq, o1 - o0);
    }
    const bool kr = a.q_off && a.kv_ragged;
    return GroupGeo{qrow0, Lqg, kr ? qrow0 : (int64_t)g * a.Lk, kr ? min(a.Lk, Lqg) : a.Lk};
}
// The rows of one 16-row query tile (first row i0 of group g, head h) as a kernel's prologue needs them: i = this lane's row inside
// the group (operand row and output row), iv = the group has it; prow = first element of its row of P / bias / dscore, drow = of
// the row its dropout draws are keyed by (a ragged group draws like the unragged layout: ortk_attn_args.drop_rows); f = its row
// fragments of `src` (Q in the forward, dO in the backward; a void pointer: the kernel takes them from an image) and k4 = its row of `keys`
// (bias; saved P), both zero for a row the group does not have.  Every load is only requested here.
template <int NJT, int NKS> struct TileRows { bool iv; int64_t prow, drow; bf16x8 f[NKS]; float4 k4[NJT]; };
template <bool OFF32, int NJT, int NKS, typename TQ>
__device__ __forceinline__ TileRows<NJT, NKS> tile_rows(const ortk_attn_args& a, const GroupGeo& gg, int g, int h, int i0, int lane,
                                                        const TQ* src, int64_t ld, const float* keys, bool keys_on) {
    TileRows<NJT, NKS> t;
    const int lr = lane & 15, lq = lane >> 4, Lq = a.Lq, Lk = a.Lk;
    const int i = i0 + lr;
    t.iv = i < gg.Lqg;
    t.prow = (((int64_t)g * a.H + h) * Lq + i) * Lk;
    t.drow = t.prow;
    if (a.drop_p > 0.f && a.drop_rows && a.q_off && t.iv)
        t.drow = (((int64_t)g * a.H + h) * Lq + ((int64_t)a.drop_rows[gg.qrow0 + i] - (int64_t)g * Lq)) * Lk;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) t.f[ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (!std::is_void<TQ>::value) {
        if (t.iv) {                                 // (OFF32: see row_off)
            const TQ* p = OFF32 ? src + gg.qrow0 * ld + h * (32 * NKS) + row_off<true>(i, ld, 8 * lq) : src + (gg.qrow0 + i) * ld + h * (32 * NKS) + 8 * lq;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) t.f[ks] = ld_frag(p + 32 * ks);
        }
    }
    ld_keys4<NJT>(t.k4, keys, keys_on && t.iv, t.prow, Lk, lq);
    return t;
}

// ------------------------------------------------------------------------------------------------ forward
// One 16-row query tile of one (group, head), by one wave: scores, mask / causal / bias, soft-max, P store, dropout, P.V.
// kfr = the K row fragments; sMask[j] = key mask (-1: padded key); sV = [KJ][PD] image of V, zero-padded; sP = this wave's
// [16][PJ] image, key columns 16*NJT .. KJ-1 zero.  i = this lane's query row inside the group, iv = it exists; prow / drow =
// first element of its P row / of the row its dropout draws are keyed by; orow = its row of O.
template <int NJT, int DKT, int PJ, typename KF>
__device__ __forceinline__ void fwd16_tile(const ortk_attn_args& a, const KF& kfr, const bf16x8 (&qf)[DKT / 32], const float4 (&bias4)[NJT],
                                           const float* sMask, const __bf16* sV, __bf16* sP, int lane, int i, bool iv,
                                           int64_t prow, int64_t drow, int64_t orow, int h, float inv_keep) {
    constexpr int DK = DKT, PD = DKT + 8, KJ = KeyGeo<NJT>::KJ;
    const float qscale = DKT == 64 ? 0.125f : 0.17677669529663687f;      // 1 / sqrt(dk)
    const int lr = lane & 15, lq = lane >> 4, Lk = a.Lk;
    const bool vec_p = (Lk & 3) == 0;               // P / bias rows start 16-byte aligned
    // S^T[j = 16*jt + 4*lq + r][i = lr]
    f32x4 s[NJT];
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt) {
        s[jt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < DK / 32; ++ks) s[jt] = mma(kfr(jt, ks), qf[ks], s[jt]);
    }
    const int qpos = a.causal_period > 0 ? i % a.causal_period : 0;
    float mx = -INFINITY;
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt) {
        const int j0 = 16 * jt + 4 * lq;
        const float bb[4] = {bias4[jt].x, bias4[jt].y, bias4[jt].z, bias4[jt].w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + r;
            const float mk = sMask[j];
            float x = s[jt][r] * qscale;
            if (mk == 0.f || (a.causal_period > 0 && j > qpos)) x = -1e9f;
            if (mk < 0.f) x = -INFINITY;                                      // padded key: not part of the row
            else if (a.bias && iv) x = bb[r] + x;
            s[jt][r] = x;
            mx = fmaxf(mx, x);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64)); mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float e = expf(s[jt][r] - mx); s[jt][r] = e; sum += e; }
    sum += __shfl_xor(sum, 16, 64); sum += __shfl_xor(sum, 32, 64);
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt) {
        const int j0 = 16 * jt + 4 * lq;
        float p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = (iv && j0 + r < Lk) ? s[jt][r] / sum : 0.f;
        if (a.p && iv) {
            if (vec_p && j0 < Lk) *reinterpret_cast<float4*>(a.p + prow + j0) = make_float4(p[0], p[1], p[2], p[3]);
            else for (int r = 0; r < 4; ++r) if (j0 + r < Lk) a.p[prow + j0 + r] = p[r];
        }
        if (a.drop_p > 0.f) {
            bool kp[4];
            ortk_keep4(a.drop_seed, (uint64_t)(drow + j0), a.drop_p, kp);
#pragma unroll
            for (int r = 0; r < 4; ++r) p[r] = kp[r] ? p[r] * inv_keep : 0.f;
        }
        *reinterpret_cast<bf16x4*>(sP + lr * PJ + j0) = cvt4(make_float4(p[0], p[1], p[2], p[3]));
    }
    wsync();
    // O^T[d = 16*dt + 4*lq + r][i = lr] = sum_j V[j][d] Pd[i][j]
    bf16x8 pf[KJ / 32];
#pragma unroll
    for (int ks = 0; ks < KJ / 32; ++ks) pf[ks] = frag_row<PJ>(sP, lr, 32 * ks + 8 * lq);
#pragma unroll
    for (int dt = 0; dt < DK / 16; ++dt) {
        f32x4 o = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KJ / 32; ++ks) o = mma(frag_tr<PD>(sV, 32 * ks, 16 * dt, lane), pf[ks], o);
        if (iv) st_elem4(a.o, orow * a.ldo + h * DK + 16 * dt + 4 * lq, a.o_dtype, make_float4(o[0], o[1], o[2], o[3]));
    }
}

// The wave-per-tile kernel: one workgroup per (group g, head h); one wave per 16-row query tile.  NJT = key tiles (Lk <= 16 * NJT <= 128).
template <int NJT, typename TQ, int DKT>
__global__ __launch_bounds__(512) void attn16_fwd_kernel(ortk_attn_args a) {
    constexpr int DK = DKT, PD = DKT + 8;           // features per head; pitch of the [row][feature] images
    const TQ* aq = reinterpret_cast<const TQ*>(a.q); const TQ* ak = reinterpret_cast<const TQ*>(a.k); const TQ* av = reinterpret_cast<const TQ*>(a.v);
    extern __shared__ __attribute__((aligned(16))) __bf16 sm16[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int g = blockIdx.x / a.H, h = blockIdx.x - g * a.H;
    constexpr int KJ = KeyGeo<NJT>::KJ, PJ = KeyGeo<NJT>::PJ;
    const Fwd16Lds L(NJT, DKT, nw);
    __bf16* sK = sm16;                              // [16*NJT][PD]   rows = key            (row fragments)
    __bf16* sV = sm16 + L.V;                        // [KJ][PD]       rows = key, zero-padded (k of P.V: transposing reads)
    __bf16* sP = sm16 + L.P + wave * 16 * PJ;       // [16][PJ]       this wave's dropped P: rows = query, columns = key 0..KJ-1
    float* sMask = reinterpret_cast<float*>(sm16 + L.mask);   // [128]
    const int lr = lane & 15, lq = lane >> 4;
    const GroupGeo gg = group_geo(a, g);
    // The launcher gives every 16-row query tile its own wave.  This wave's Q fragments and bias rows are requested BEFORE
    // the K / V staging and its barrier, so that the workgroup pays one global round trip, not two.
    const int i = wave * 16 + lr;                   // this lane's query row inside the group (operand row and output row)
    const TileRows<NJT, DK / 32> t = tile_rows<false, NJT, DK / 32>(a, gg, g, h, wave * 16, lane, aq, a.ldq, a.bias, a.bias != nullptr);
    stage_rows<DK>(sK, ak + gg.krow0 * a.ldk + h * DK, a.ldk, gg.Lkg, 16 * NJT, tid, blockDim.x);
    stage_rows<DK>(sV, av + gg.krow0 * a.ldv + h * DK, a.ldv, gg.Lkg, KJ, tid, blockDim.x);
    for (int j = tid; j < 128; j += blockDim.x)     // all 128 entries whatever the workgroup size (one wave when Lq <= 16)
        sMask[j] = (j < gg.Lkg) ? (a.kmask ? a.kmask[gg.krow0 + j] : 1.f) : -1.f;              // -1: padded key
    zero_cols<PJ, KJ>(sP, 16, lane, 64);
    __syncthreads();
    const float inv_keep = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
    if (wave * 16 < a.Lq)
        fwd16_tile<NJT, DKT, PJ>(a, LdsRowFrags<PD>{sK, lr, lq}, t.f, t.k4, sMask, sV, sP, lane, i, t.iv, t.prow, t.drow, gg.qrow0 + i, h, inv_keep);
}

// The short kernel (bf16 Q / K / V, Lq <= 32, Lk <= 32: the decoder's causal self-attention): one WAVE per (group, head), pair
// p = blockIdx.x * W + wave, so the heads of a group sit in adjacent waves and a workgroup reads whole neighbouring lines of the
// packed rows.  The wave runs the query tiles that hold rows of its group one after the other (captions of at most 16 rows: one).
// K goes from global memory straight into row fragments; LDS holds, per wave, the V image (transposing reads), the P image
// (C-layout -> operand) and the 32 key-mask entries: 6 016 B at dk = 64.  Every global load is issued before the first wait;
// no __syncthreads(): a wave only ever touches its own LDS region.
template <int NJT, int DKT>
__global__ __launch_bounds__(512) void attn16s_fwd_kernel(ortk_attn_args a) {
    static_assert(NJT <= 2, "the short kernels serve at most 32 keys");
    constexpr int DK = DKT, NKS = DKT / 32;
    const __bf16* aq = reinterpret_cast<const __bf16*>(a.q); const __bf16* ak = reinterpret_cast<const __bf16*>(a.k); const __bf16* av = reinterpret_cast<const __bf16*>(a.v);
    extern __shared__ __attribute__((aligned(16))) __bf16 sm16[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), W = blockDim.x >> 6;
    const int pair = blockIdx.x * W + wave;
    if (pair >= a.nkv * a.H) return;                // the last workgroup may be partly empty (no workgroup barrier below)
    const int g = pair / a.H, h = pair - g * a.H;
    constexpr Fwd16sLds L(DKT);
    __bf16* sV = sm16 + wave * L.end;                          // [KJS][PD]  rows = key, zero-padded
    __bf16* sP = sV + L.P;                                     // [16][PJS]  dropped P of the current tile
    float* sMask = reinterpret_cast<float*>(sV + L.mask);      // [32]
    const int lr = lane & 15;
    const GroupGeo gg = group_geo(a, g);
    // ---- every global load of the wave
    bf16x8 vreg[Stage<DKT, KJS, 64>::N];
    stage_ld<DKT, KJS, 64>(vreg, av + gg.krow0 * a.ldv + h * DK, a.ldv, gg.Lkg, lane);
    const float mk = (lane < gg.Lkg) ? (a.kmask ? a.kmask[gg.krow0 + lane] : 1.f) : -1.f;  // -1: padded key (Lkg <= 32: lanes 0 .. 31 are stored)
    RegRowFrags<NJT, NKS> kf;
    ld_row_frags<false>(kf, ak + gg.krow0 * a.ldk + h * DK, a.ldk, gg.Lkg, lane);
    TileRows<NJT, NKS> t[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) t[it] = tile_rows<false, NJT, NKS>(a, gg, g, h, it * 16, lane, aq, a.ldq, a.bias, a.bias != nullptr);
    // ---- the wave's LDS region
    stage_st<DKT, KJS, 64>(sV, vreg, KJS, lane);
    if (lane < 32) sMask[lane] = mk;
    zero_cols<PJS, KJS>(sP, 16, lane, 64);
    wsync();
    const float inv_keep = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        if (it * 16 >= gg.Lqg) break;               // a tile with no row of the group stores nothing
        fwd16_tile<NJT, DKT, PJS>(a, kf, t[it].f, t[it].k4, sMask, sV, sP, lane, it * 16 + lr, t[it].iv, t[it].prow, t[it].drow,
                                  gg.qrow0 + it * 16 + lr, h, inv_keep);
        wsync();                                    // the next tile overwrites the P image
    }
}

// The second mapping of the block kernels (ortk_tuning.attn16_block; bf16 Q / K / V, at most 64 keys and 96 query rows): still a
// workgroup per (group, head), but sized by how many of them a compute unit holds side by side, not by one wave per query tile.
// A workgroup is one latency chain (offsets -> global loads -> LDS images -> barrier -> MFMA, soft-max, MFMA -> stores); 2 048 of
// them run in rounds, and LDS sets the round size.  Three waves whatever Lq: wave w runs query tiles w and, past 48 rows, w + 3
// (one P image, reused behind a wsync(); a tile with no row of a ragged group is skipped).  The K image lives only until every wave
// has taken its row fragments into registers; behind one more barrier its bytes are the three P images, so LDS holds the V image,
// that region and the key mask: 16 384 B at 36 keys and dk = 64 (23 552 / 30 464 B in attn16_fwd_kernel).  K goes through LDS and
// not straight into fragments (as in the short kernel) because 24 more registers in flight beside the V, Q and bias loads do not
// fit the 80 of 6 waves per SIMD.  Every global load is issued before the first wait.
// (registers: 6 waves per SIMD = 8 workgroups per compute unit; 4 key tiles at dk = 64 do not fit 80 registers and get 128)
template <int NJT, int DKT, int TPW>
__global__ __launch_bounds__(NTB) __attribute__((amdgpu_waves_per_eu(NJT * DKT > 192 ? 4 : 6))) void attn16b_fwd_kernel(ortk_attn_args a) {
    static_assert(NJT <= 4 && TPW <= 2, "at most 64 keys and 96 query rows");
    constexpr int DK = DKT, PD = DKT + 8, NKS = DKT / 32, KJ = KeyGeo<NJT>::KJ, PJ = KeyGeo<NJT>::PJ;
    const __bf16* aq = reinterpret_cast<const __bf16*>(a.q); const __bf16* ak = reinterpret_cast<const __bf16*>(a.k); const __bf16* av = reinterpret_cast<const __bf16*>(a.v);
    extern __shared__ __attribute__((aligned(16))) __bf16 sm16[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = blockIdx.x / a.H, h = blockIdx.x - g * a.H;
    constexpr Fwd16bLds L(NJT, DKT);
    __bf16* sV = sm16;                                         // [KJ][PD]      rows = key, zero-padded
    __bf16* sK = sm16 + L.K;                                   // [16*NJT][PD]  rows = key: on its way into every wave's row fragments
    __bf16* sP = sK + wave * 16 * PJ;                          // [16][PJ]      then this wave's dropped P of the current tile
    float* sMask = reinterpret_cast<float*>(sm16 + L.mask);    // [64]
    const int lr = lane & 15, lq = lane >> 4;
    const GroupGeo gg = group_geo(a, g);
    // ---- every global load of the workgroup
    bf16x8 vreg[Stage<DKT, KJ, NTB>::N];
    stage_ld<DKT, KJ, NTB>(vreg, av + gg.krow0 * a.ldv + h * DK, a.ldv, gg.Lkg, tid);
    float mk = -1.f;                                // -1: padded key
    if (tid < gg.Lkg) mk = a.kmask ? a.kmask[gg.krow0 + tid] : 1.f;              // (Lkg <= 64: threads 0 .. 63 are stored)
    bf16x8 kreg[Stage<DKT, 16 * NJT, NTB>::N];
    stage_ld<DKT, 16 * NJT, NTB>(kreg, ak + gg.krow0 * a.ldk + h * DK, a.ldk, gg.Lkg, tid);
    TileRows<NJT, NKS> t[TPW];
    if constexpr (TPW == 1) {
        t[0] = tile_rows<true, NJT, NKS>(a, gg, g, h, wave * 16, lane, aq, a.ldq, a.bias, a.bias != nullptr);
    } else {
        // tile_rows written out: through the shared function the two-tile instances <3,64,2> and <4,32,2> spill 12 and 20 bytes
        // (profiles/attention_refactor.txt); a wave that runs two tiles loads no bias (see attn16_plan)
#pragma unroll
        for (int k = 0; k < TPW; ++k) {
            const int i = (wave + NWB * k) * 16 + lr, lq = lane >> 4;
            t[k].iv = i < gg.Lqg;
            t[k].prow = (((int64_t)g * a.H + h) * a.Lq + i) * a.Lk;
            t[k].drow = t[k].prow;
            if (a.drop_p > 0.f && a.drop_rows && a.q_off && t[k].iv)
                t[k].drow = (((int64_t)g * a.H + h) * a.Lq + ((int64_t)a.drop_rows[gg.qrow0 + i] - (int64_t)g * a.Lq)) * a.Lk;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) t[k].f[ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
            if (t[k].iv) {
                const __bf16* p = aq + gg.qrow0 * a.ldq + h * DK + row_off<true>(i, a.ldq, 8 * lq);
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) t[k].f[ks] = ld_frag(p + 32 * ks);
            }
            ld_keys4<NJT>(t[k].k4, a.bias, false && t[k].iv, t[k].prow, a.Lk, lq);
        }
    }
    // ---- the images
    stage_st<DKT, KJ, NTB>(sV, vreg, KJ, tid);
    stage_st<DKT, 16 * NJT, NTB>(sK, kreg, 16 * NJT, tid);
    if (tid < 64) sMask[tid] = mk;
    __syncthreads();
    // every wave takes the whole of K as row fragments (what LdsRowFrags would read tile by tile), then the image's bytes are the P images
    RegRowFrags<NJT, NKS> kf;
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) kf.f[jt][ks] = frag_row<PD>(sK, 16 * jt + lr, 32 * ks + 8 * lq);
    __syncthreads();
    zero_cols<PJ, KJ>(sP, 16, lane, 64);
    const float inv_keep = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
        const int i0 = (wave + NWB * k) * 16;
        if (i0 >= gg.Lqg) break;                    // a tile with no row of the group stores nothing
        if (k) wsync();                             // this tile overwrites the P image
        fwd16_tile<NJT, DKT, PJ>(a, kf, t[k].f, t[k].k4, sMask, sV, sP, lane, i0 + lr, t[k].iv, t[k].prow, t[k].drow, gg.qrow0 + i0 + lr, h, inv_keep);
    }
}

// ------------------------------------------------------------------------------------------------ backward
// Phase 1 (wave = 16-row query tile): dP^T = V dO^T, dS = P (dP - rowsum(P dP)), dQ = dS K / sqrt(dk); dS / sqrt(dk) and the
// dropped P go to workgroup-wide images.  Phase 2 (the 2 x NJT x 4 output tiles shared by the waves): dK = dS^T Q / sqrt(dk),
// dV = Pd^T dO over all query rows of the group.  Lqp = query rows padded to a multiple of 32 (k range of phase 2).
//
// Phase 1 for one 16-row query tile of one (group, head), by one wave.  vfr = the V row fragments, gf = this lane's dO row
// fragments, praw = its saved P row; sK = [KJ][PD] image of K, zero-padded; sS / sD = the [query][key] images of the group (row
// i = this lane's query row inside the group; key columns 16*NJT .. KJ-1 zero).  prow / drow / qrow as in fwd16_tile.
template <int NJT, int DKT, int PJ, typename VF>
__device__ __forceinline__ void bwd16_tile1(const ortk_attn_args& a, const VF& vfr, const bf16x8 (&gf)[DKT / 32], const float4 (&praw)[NJT],
                                            const __bf16* sK, __bf16* sS, __bf16* sD, int lane, int i, bool iv,
                                            int64_t prow, int64_t drow, int64_t qrow, int h, float inv_keep) {
    constexpr int DK = DKT, PD = DKT + 8, KJ = KeyGeo<NJT>::KJ;
    const float qscale = DKT == 64 ? 0.125f : 0.17677669529663687f;
    const int lq = lane >> 4, Lk = a.Lk;
    const bool vec_p = (Lk & 3) == 0;
    // dP^T[j = 16*jt + 4*lq + r][i = lr]
    f32x4 dp[NJT], pp[NJT];
    float dot = 0.f;
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt) {
        dp[jt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < DK / 32; ++ks) dp[jt] = mma(vfr(jt, ks), gf[ks], dp[jt]);
        const int j0 = 16 * jt + 4 * lq;
        const float pv[4] = {praw[jt].x, praw[jt].y, praw[jt].z, praw[jt].w};
        float pd[4];
        bool kp[4] = {true, true, true, true};
        if (a.drop_p > 0.f) ortk_keep4(a.drop_seed, (uint64_t)(drow + j0), a.drop_p, kp);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool valid = iv && j0 + r < Lk;
            const bool keep = valid && kp[r];
            const float d = keep ? dp[jt][r] * inv_keep : 0.f;
            pd[r] = keep ? pv[r] * inv_keep : 0.f;
            pp[jt][r] = valid ? pv[r] : 0.f; dp[jt][r] = d; dot += pp[jt][r] * d;
        }
        *reinterpret_cast<bf16x4*>(sD + i * PJ + j0) = cvt4(make_float4(pd[0], pd[1], pd[2], pd[3]));
    }
    dot += __shfl_xor(dot, 16, 64); dot += __shfl_xor(dot, 32, 64);
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt) {
        const int j0 = 16 * jt + 4 * lq;
        float ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ds[r] = pp[jt][r] * (dp[jt][r] - dot);
        if (a.dscore && iv) {
            if (vec_p && j0 < Lk) *reinterpret_cast<float4*>(a.dscore + prow + j0) = make_float4(ds[0], ds[1], ds[2], ds[3]);
            else for (int r = 0; r < 4; ++r) if (j0 + r < Lk) a.dscore[prow + j0 + r] = ds[r];
        }
        *reinterpret_cast<bf16x4*>(sS + i * PJ + j0) = cvt4(make_float4(ds[0] * qscale, ds[1] * qscale, ds[2] * qscale, ds[3] * qscale));
    }
    wsync();
    // dQ^T[d = 16*dt + 4*lq + r][i = lr] = sum_j K[j][d] dSs[i][j]
    bf16x8 sf[KJ / 32];
#pragma unroll
    for (int ks = 0; ks < KJ / 32; ++ks) sf[ks] = frag_row<PJ>(sS, i, 32 * ks + 8 * lq);
#pragma unroll
    for (int dt = 0; dt < DK / 16; ++dt) {
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KJ / 32; ++ks) acc = mma(frag_tr<PD>(sK, 32 * ks, 16 * dt, lane), sf[ks], acc);
        if (iv) st_elem4(a.dq, qrow * a.lddq + h * DK + 16 * dt + 4 * lq, a.dqkv_dtype, make_float4(acc[0], acc[1], acc[2], acc[3]));
    }
}
// Phase 2, output tile t = (which, jt, dt) of one (group, head), by one wave:
// D[d = 16*dt + 4*lq + r][j = 16*jt + lr] = sum_i B[i][d] A[i][j], (A, B) = (dS, Q) for dK and (dropped P, dO) for dV
template <int NJT, int DKT, int PJ>
__device__ __forceinline__ void bwd16_tile2(const ortk_attn_args& a, int t, const __bf16* sS, const __bf16* sD, const __bf16* sQ, const __bf16* sG,
                                            int Lqp, int lane, int Lkg, int64_t krow0, int h) {
    constexpr int DK = DKT, PD = DKT + 8, NDT = DK / 16;
    const int lr = lane & 15, lq = lane >> 4;
    const int which = t / (NJT * NDT), rem = t - which * NJT * NDT, jt = rem / NDT, dt = rem % NDT;
    const __bf16* sA = which == 0 ? sS : sD;      // [query][key]
    const __bf16* sB = which == 0 ? sQ : sG;      // [query][feature]
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < Lqp; k0 += 32) acc = mma(frag_tr<PD>(sB, k0, 16 * dt, lane), frag_tr<PJ>(sA, k0, 16 * jt, lane), acc);
    const int j = 16 * jt + lr;
    if (j < Lkg) {
        const int64_t row = krow0 + j;
        const float4 v = make_float4(acc[0], acc[1], acc[2], acc[3]);
        if (which == 0) st_elem4(a.d_k, row * a.lddk + h * DK + 16 * dt + 4 * lq, a.dqkv_dtype, v);
        else            st_elem4(a.dv, row * a.lddv + h * DK + 16 * dt + 4 * lq, a.dqkv_dtype, v);
    }
}

// The wave-per-tile kernel: one workgroup per (group g, head h); phase 1 with one wave per query tile, phase 2 shared by the waves.
template <int NJT, typename TQ, int DKT>
__global__ __launch_bounds__(512) void attn16_bwd_kernel(ortk_attn_args a, int Lqp) {
    constexpr int DK = DKT, PD = DKT + 8;
    const TQ* aq = reinterpret_cast<const TQ*>(a.q); const TQ* ak = reinterpret_cast<const TQ*>(a.k); const TQ* av = reinterpret_cast<const TQ*>(a.v);
    extern __shared__ __attribute__((aligned(16))) __bf16 sm16[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int g = blockIdx.x / a.H, h = blockIdx.x - g * a.H;
    constexpr int KJ = KeyGeo<NJT>::KJ, PJ = KeyGeo<NJT>::PJ;
    const Bwd16Lds L(NJT, DKT, Lqp);
    __bf16* sK = sm16;                      // [KJ][PD]       rows = key, zero-padded   (k of dS.K: transposing reads)
    __bf16* sV = sm16 + L.V;                // [16*NJT][PD]   rows = key                (row fragments of dP^T = V dO^T)
    __bf16* sQ = sm16 + L.Q;                // [Lqp][PD]      rows = query              (k of dS^T Q: transposing reads)
    __bf16* sG = sm16 + L.G;                // [Lqp][PD]      dO: row fragments in phase 1, transposing reads in phase 2
    __bf16* sS = sm16 + L.S;                // [Lqp][PJ]      dS / sqrt(dk): rows = query, columns = key 0..KJ-1
    __bf16* sD = sm16 + L.D;                // [Lqp][PJ]      dropped P (follows sS)
    const int lr = lane & 15, lq = lane >> 4;
    // Query rows past a ragged group's count are staged as ZERO rows of Q and dO (they are another group's rows): they add
    // nothing to dK / dV
    const GroupGeo gg = group_geo(a, g);
    // one 16-row query tile per wave; its saved probabilities are requested before the staging barrier (its dO fragments come
    // from the image: the inputs may be fp32)
    const int i = wave * 16 + lr;                   // this lane's query row inside the group (operand row and output row)
    TileRows<NJT, DK / 32> t = tile_rows<false, NJT, DK / 32>(a, gg, g, h, wave * 16, lane, (const void*)nullptr, 0, a.p, true);
    stage_rows<DK>(sK, ak + gg.krow0 * a.ldk + h * DK, a.ldk, gg.Lkg, KJ, tid, blockDim.x);
    stage_rows<DK>(sV, av + gg.krow0 * a.ldv + h * DK, a.ldv, gg.Lkg, 16 * NJT, tid, blockDim.x);
    stage_rows<DK>(sQ, aq + gg.qrow0 * a.ldq + h * DK, a.ldq, gg.Lqg, Lqp, tid, blockDim.x);
    stage_rows<DK>(sG, reinterpret_cast<const TQ*>(a.d_o) + gg.qrow0 * a.lddo + h * DK, a.lddo, gg.Lqg, Lqp, tid, blockDim.x);
    zero_cols<PJ, KJ>(sS, 2 * Lqp, tid, blockDim.x);      // (both images: also the query rows past the last wave tile)
    __syncthreads();
    const float inv_keep = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
    if (wave * 16 < a.Lq) {
#pragma unroll
        for (int ks = 0; ks < DK / 32; ++ks) t.f[ks] = frag_row<PD>(sG, i, 32 * ks + 8 * lq);
        bwd16_tile1<NJT, DKT, PJ>(a, LdsRowFrags<PD>{sV, lr, lq}, t.f, t.k4, sK, sS, sD, lane, i, t.iv, t.prow, t.drow, gg.qrow0 + i, h, inv_keep);
    }
    __syncthreads();
    for (int k = wave; k < 2 * NJT * (DK / 16); k += nw) bwd16_tile2<NJT, DKT, PJ>(a, k, sS, sD, sQ, sG, Lqp, lane, gg.Lkg, gg.krow0, h);
}

// The short kernel: the mapping of attn16s_fwd_kernel.  One wave runs phase 1 for the query tiles that hold rows of its group,
// then the 2 x NJT x (dk / 16) tiles of phase 2.  V and dO reach dP^T = V dO^T as row fragments straight from global memory; LDS
// holds, per wave, the dS / P images (C-layout -> operand; 32 query rows, pitch PJS) and ONE [32][PD] image for the operand a
// transposing read needs next: K for dQ, then Q for the dK tiles, then dO for the dV tiles (Q and dO wait in registers, where
// their loads left them): 9 728 B at dk = 64, 16 waves per compute unit.  Key tiles past the group's keys (a caption of at most
// 16 rows: tile 1) have no row of dK / dV to store and are skipped.
template <int NJT, int DKT>
__global__ __launch_bounds__(512) void attn16s_bwd_kernel(ortk_attn_args a) {
    static_assert(NJT <= 2, "the short kernels serve at most 32 keys");
    constexpr int DK = DKT, NKS = DKT / 32, LQP = 32;
    const __bf16* aq = reinterpret_cast<const __bf16*>(a.q); const __bf16* ak = reinterpret_cast<const __bf16*>(a.k); const __bf16* av = reinterpret_cast<const __bf16*>(a.v);
    const __bf16* ag = reinterpret_cast<const __bf16*>(a.d_o);
    extern __shared__ __attribute__((aligned(16))) __bf16 sm16[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), W = blockDim.x >> 6;
    const int pair = blockIdx.x * W + wave;
    if (pair >= a.nkv * a.H) return;                // the last workgroup may be partly empty (no workgroup barrier below)
    const int g = pair / a.H, h = pair - g * a.H;
    constexpr Bwd16sLds L(DKT);
    __bf16* sX = sm16 + wave * L.end;                          // [32][PD]    K (rows = key), then Q, then dO (rows = query); zero-padded
    __bf16* sS = sX + L.S;                                     // [LQP][PJS]  dS / sqrt(dk)
    __bf16* sD = sX + L.D;                                     // [LQP][PJS]  dropped P (follows sS)
    const int lr = lane & 15;
    const GroupGeo gg = group_geo(a, g);
    // ---- every global load of the wave: what phase 1 consumes from registers first, then the three staged images
    RegRowFrags<NJT, NKS> vf;
    ld_row_frags<false>(vf, av + gg.krow0 * a.ldv + h * DK, a.ldv, gg.Lkg, lane);
    TileRows<NJT, NKS> t[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) t[it] = tile_rows<false, NJT, NKS>(a, gg, g, h, it * 16, lane, ag, a.lddo, a.p, true);
    bf16x8 kreg[Stage<DKT, 32, 64>::N], qreg[Stage<DKT, 32, 64>::N], greg[Stage<DKT, 32, 64>::N];
    stage_ld<DKT, 32, 64>(kreg, ak + gg.krow0 * a.ldk + h * DK, a.ldk, gg.Lkg, lane);
    stage_ld<DKT, 32, 64>(qreg, aq + gg.qrow0 * a.ldq + h * DK, a.ldq, gg.Lqg, lane);
    stage_ld<DKT, 32, 64>(greg, ag + gg.qrow0 * a.lddo + h * DK, a.lddo, gg.Lqg, lane);
    // ---- the wave's LDS region
    zero_cols<PJS, PJS>(sS, 2 * LQP, lane, 64);
    stage_st<DKT, 32, 64>(sX, kreg, 32, lane);
    wsync();
    const float inv_keep = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        if (it * 16 >= gg.Lqg) break;               // a tile with no row of the group: zero rows of dS / P, nothing stored
        bwd16_tile1<NJT, DKT, PJS>(a, vf, t[it].f, t[it].k4, sX, sS, sD, lane, it * 16 + lr, t[it].iv, t[it].prow, t[it].drow,
                                   gg.qrow0 + it * 16 + lr, h, inv_keep);
    }
    // phase 2: tile t = (which, jt, dt); which = 0 the dK tiles (dS, Q), 1 the dV tiles (dropped P, dO)
    constexpr int NDT = DK / 16;
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        wsync();                                    // the image's readers (dQ; the dK tiles) are done, and dS / P are whole
        stage_st<DKT, 32, 64>(sX, which == 0 ? qreg : greg, 32, lane);
        wsync();
        for (int jt = 0; jt < NJT && 16 * jt < gg.Lkg; ++jt)
            for (int dt = 0; dt < NDT; ++dt)
                bwd16_tile2<NJT, DKT, PJS>(a, (which * NJT + jt) * NDT + dt, sS, sD, sX, sX, LQP, lane, gg.Lkg, gg.krow0, h);
    }
}

// The second mapping of the block backward (see attn16b_fwd_kernel): the layout of attn16s_bwd_kernel, workgroup-wide.  V and dO
// reach dP^T = V dO^T as row fragments straight from global memory; LDS holds the dS / P images of the group and ONE
// [max(KJ, Lqp)][PD] image for the operand a transposing read needs next: K for dQ, then Q for the dK tiles, then dO for the dV
// tiles (Q and dO wait in the registers their loads filled; the hand-overs are workgroup barriers): 27 648 B for 36 x 36 and
// 41 472 B for 85 x 36 at dk = 64 (52 992 / 71 424 B in attn16_bwd_kernel).  Phase 2 stops its k loop at the last 32-row block
// that holds a row of the group (zero rows add +0 to an accumulator that started at +0: the same bits).
template <int NJT, int DKT, int TPW>
__global__ __launch_bounds__(NTB) void attn16b_bwd_kernel(ortk_attn_args a, int Lqp) {
    static_assert(NJT <= 4 && TPW <= 2, "at most 64 keys and 96 query rows");
    constexpr int DK = DKT, PD = DKT + 8, NKS = DKT / 32, KJ = KeyGeo<NJT>::KJ, PJ = KeyGeo<NJT>::PJ;
    constexpr int LQM = TPW == 1 ? 64 : 96;         // Lqp of the instance's longest query block (48 | 96 rows)
    const __bf16* aq = reinterpret_cast<const __bf16*>(a.q); const __bf16* ak = reinterpret_cast<const __bf16*>(a.k); const __bf16* av = reinterpret_cast<const __bf16*>(a.v);
    const __bf16* ag = reinterpret_cast<const __bf16*>(a.d_o);
    extern __shared__ __attribute__((aligned(16))) __bf16 sm16[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = blockIdx.x / a.H, h = blockIdx.x - g * a.H;
    // This kernel keeps its own spelling of the geometry (group_geo), the row setup (tile_rows), the image clear (zero_cols) and the
    // carve (Bwd16bLds, which attn16_plan sizes the launch by): with the shared pieces its instance <1,32,2> went from 74 to 78
    // registers and from 6 to 5 waves per SIMD, whichever of them was tried alone (profiles/attention_refactor.txt).
    const int Lk = a.Lk, Lq = a.Lq;
    __bf16* sX = sm16;                              // [max(KJ, Lqp)][PD]  K (rows = key), then Q, then dO (rows = query); zero-padded
    __bf16* sS = sX + max(KJ, Lqp) * PD;            // [Lqp][PJ]           dS / sqrt(dk)
    __bf16* sD = sS + Lqp * PJ;                     // [Lqp][PJ]           dropped P
    const int lr = lane & 15, lq = lane >> 4;
    int64_t qrow0 = (int64_t)g * Lq;
    int Lqg = Lq;
    if (a.q_off) {
        const int o0 = a.q_off[(int64_t)g * a.q_off_stride], o1 = a.q_off[(int64_t)(g + 1) * a.q_off_stride];
        qrow0 = o0; Lqg = min(Lq, o1 - o0);
    }
    const int64_t krow0 = (a.q_off && a.kv_ragged) ? qrow0 : (int64_t)g * Lk;
    const int Lkg = (a.q_off && a.kv_ragged) ? min(Lk, Lqg) : Lk;
    // ---- every global load of the workgroup: what phase 1 consumes from registers first, then the three staged images
    RegRowFrags<NJT, NKS> vf;
    ld_row_frags<true>(vf, av + krow0 * a.ldv + h * DK, a.ldv, Lkg, lane);
    bf16x8 gf[TPW][NKS];
    float4 praw[TPW][NJT];
    int64_t prow[TPW], drow[TPW];
    bool iv[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int i = (wave + NWB * t) * 16 + lr;
        iv[t] = i < Lqg;
        prow[t] = (((int64_t)g * a.H + h) * Lq + i) * Lk;
        drow[t] = prow[t];
        if (a.drop_p > 0.f && a.drop_rows && a.q_off && iv[t])
            drow[t] = (((int64_t)g * a.H + h) * Lq + ((int64_t)a.drop_rows[qrow0 + i] - (int64_t)g * Lq)) * Lk;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) gf[t][ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};        // (a zero row of the dO image)
        if (iv[t]) {
            const __bf16* gp = ag + qrow0 * a.lddo + h * DK + ((unsigned)i * (unsigned)a.lddo + (unsigned)(8 * lq));
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) gf[t][ks] = ld_frag(gp + 32 * ks);
        }
        ld_keys4<NJT>(praw[t], a.p, iv[t], prow[t], Lk, lq);
    }
    bf16x8 kreg[Stage<DKT, KJ, NTB>::N], qreg[Stage<DKT, LQM, NTB>::N], greg[Stage<DKT, LQM, NTB>::N];
    stage_ld<DKT, KJ, NTB>(kreg, ak + krow0 * a.ldk + h * DK, a.ldk, Lkg, tid);
    stage_ld<DKT, LQM, NTB>(qreg, aq + qrow0 * a.ldq + h * DK, a.ldq, Lqg, tid);
    stage_ld<DKT, LQM, NTB>(greg, ag + qrow0 * a.lddo + h * DK, a.lddo, Lqg, tid);
    // ---- the images.  dS / P: key columns 16*NJT .. KJ-1 and the rows of a tile that is not run stay zero
    for (int idx = tid; idx < 2 * Lqp * PJ / 8; idx += NTB)
        *reinterpret_cast<bf16x8*>(sS + idx * 8) = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};           // sD follows sS
    stage_st<DKT, KJ, NTB>(sX, kreg, KJ, tid);
    __syncthreads();
    const float inv_keep = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int i0 = (wave + NWB * t) * 16;
        if (i0 >= Lqg) break;                       // a tile with no row of the group: zero rows of dS / P, nothing stored
        bwd16_tile1<NJT, DKT, PJ>(a, vf, gf[t], praw[t], sX, sS, sD, lane, i0 + lr, iv[t], prow[t], drow[t], qrow0 + i0 + lr, h, inv_keep);
    }
    // phase 2: tile (which, jt, dt); which = 0 the dK tiles (dS, Q), 1 the dV tiles (dropped P, dO), shared by the waves
    constexpr int NT2 = NJT * (DK / 16);
    const int Lq2 = min(Lqp, (Lqg + 31) & ~31);
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        __syncthreads();                            // the image's readers (dQ; the dK tiles) are done, and dS / P are whole
        stage_st<DKT, LQM, NTB>(sX, which == 0 ? qreg : greg, Lqp, tid);
        __syncthreads();
        for (int t = wave; t < NT2; t += NWB) bwd16_tile2<NJT, DKT, PJ>(a, which * NT2 + t, sS, sD, sX, sX, Lq2, lane, Lkg, krow0, h);
    }
}
// ------------------------------------------------------------------------------------------------ host side: this family's part of the plan
using ortk::aligned; using ortk::aligned16; using ortk::ld_multiple; using ortk::AttnInst;
typedef float f32; typedef __bf16 bf16;      // element types as the instance names spell them
#define INST(...) ORTK_ATTN_INST(, __VA_ARGS__)
#define ROW8(family, TQ, DK) {INST(family, 1,TQ,DK), INST(family, 2,TQ,DK), INST(family, 3,TQ,DK), INST(family, 4,TQ,DK), \
                              INST(family, 5,TQ,DK), INST(family, 6,TQ,DK), INST(family, 7,TQ,DK), INST(family, 8,TQ,DK)}
#define ROW4(family, DK, TPW) {INST(family, 1,DK,TPW), INST(family, 2,DK,TPW), INST(family, 3,DK,TPW), INST(family, 4,DK,TPW)}
// every instance, [backward][dk == 32]...[key tiles - 1]
const AttnInst WAVE_TILE[2][2][2][8] = {{{ROW8(attn16_fwd, f32,64), ROW8(attn16_fwd, bf16,64)}, {ROW8(attn16_fwd, f32,32), ROW8(attn16_fwd, bf16,32)}},      // [qkv_dtype]
                                        {{ROW8(attn16_bwd, f32,64), ROW8(attn16_bwd, bf16,64)}, {ROW8(attn16_bwd, f32,32), ROW8(attn16_bwd, bf16,32)}}};
const AttnInst BLOCK[2][2][2][4] = {{{ROW4(attn16b_fwd, 64,1), ROW4(attn16b_fwd, 64,2)}, {ROW4(attn16b_fwd, 32,1), ROW4(attn16b_fwd, 32,2)}},                // [tiles per wave - 1]
                                    {{ROW4(attn16b_bwd, 64,1), ROW4(attn16b_bwd, 64,2)}, {ROW4(attn16b_bwd, 32,1), ROW4(attn16b_bwd, 32,2)}}};
const AttnInst SHORT[2][2][2] = {{{INST(attn16s_fwd, 1,64), INST(attn16s_fwd, 2,64)}, {INST(attn16s_fwd, 1,32), INST(attn16s_fwd, 2,32)}},
                                 {{INST(attn16s_bwd, 1,64), INST(attn16s_bwd, 2,64)}, {INST(attn16s_bwd, 1,32), INST(attn16s_bwd, 2,32)}}};
#undef ROW4
#undef ROW8
#undef INST
static_assert(lds_bytes(Bwd16Lds(8, 64, 128)) <= 160 * 1024, "every served shape fits the LDS of a compute unit");

// layouts these kernels serve (everything else stays with the fp32-MFMA family)
bool attn16_ok(const ortk_attn_args& a, bool bwd) {
    // fp32 inputs: only the block shapes (the register-only kernels keep the short ones); bf16 inputs: every served shape
    // (short query blocks over at most 48 keys stay with the register-only kernels; past 48 keys those do not apply)
    if (a.precision != 1 || !ortk::attn16_shape_ok(a.Lq, a.Lk, a.dk) || (a.qkv_dtype == 0 && a.Lq < ortk::tuning().attn16_min_lq && a.Lk <= 48)) return false;
    if (a.kv_index || a.kv_group_stride > 0 || a.kv_dtype != 0 || a.k_new || a.v_new) return false;
    if (a.q_off && (a.qkv_dtype != 1 || a.q_off_stride < 1)) return false;
    const int in_ld = a.qkv_dtype ? 8 : 4;          // input rows (Q, K, V, dO) start 16-byte aligned
    if (!ld_multiple(in_ld, a.ldq, a.ldk, a.ldv) || !aligned16(a.q, a.k, a.v)) return false;
    if (!bwd) return ld_multiple(4, a.ldo) && aligned(a.o, a.o_dtype == ORTK_BF16 ? 8 : 16) && aligned16(a.p, a.bias);
    if (!a.p || !a.d_o || !a.dq || !a.d_k || !a.dv) return false;
    const size_t eg4 = a.dqkv_dtype == ORTK_BF16 ? 8 : 16;
    return ld_multiple(in_ld, a.lddo) && ld_multiple(4, a.lddq, a.lddk, a.lddv) && aligned16(a.d_o, a.p, a.dscore) &&
           aligned(a.dq, eg4) && aligned(a.d_k, eg4) && aligned(a.dv, eg4);
}

}  // namespace

namespace ortk {

// shapes these kernels serve
bool attn16_shape_ok(int Lq, int Lk, int dk) { return (dk == 64 || dk == 32) && Lk >= 1 && Lk <= 128 && Lq >= 1 && Lq <= 128; }

bool attn16_plan(const ortk_attn_args& a, bool bwd, AttnPlan& pl) {
    if (!attn16_ok(a, bwd)) return false;
    const int njt = (a.Lk + 15) / 16, nw = (a.Lq + 15) / 16, Lqp = (int)ortk_align(a.Lq, 32), d32 = a.dk == 32, sw = tuning().attn16_short;
    const int64_t pairs = (int64_t)a.nkv * a.H;
    auto add = [&](AttnInst k, int64_t grid, int block, size_t lds) { pl.add(k, grid, block, lds, lds > 64 * 1024 ? 160 * 1024 : 0, Lqp); };
    if (sw && a.qkv_dtype == 1 && a.Lq <= 32 && a.Lk <= 32) {
        // The short kernels (one wave per (group, head)): bf16 Q / K / V / dO, at most 32 query rows and 32 keys per group
        // (ortk_tuning.attn16_short: 0 never | 1 the default width of 4 waves per workgroup | 4, 8 that width)
        const int W = sw == 8 ? 8 : 4;
        add(SHORT[bwd][d32][njt - 1], ortk_cdiv(pairs, W), 64 * W, W * (bwd ? lds_bytes(Bwd16sLds(a.dk)) : lds_bytes(Fwd16sLds(a.dk))));
    } else if (tuning().attn16_block && a.qkv_dtype == 1 && a.Lk <= 64 && a.Lq <= 16 * NWB * 2 && (a.Lq <= 16 * NWB || !a.bias)) {
        // The block kernels (ortk_tuning.attn16_block: 1 | 0 never): bf16 Q / K / V / dO, at most 64 keys and 96 query rows: nw
        // query tiles on NWB waves, one each or two.  A biased block of more than 48 query rows stays with the wave-per-tile kernels:
        // the two bias rows of a wave that runs two tiles do not fit its registers, and the step has no such block.
        add(BLOCK[bwd][d32][nw > NWB][njt - 1], pairs, NTB, bwd ? lds_bytes(Bwd16bLds(njt, a.dk, Lqp)) : lds_bytes(Fwd16bLds(njt, a.dk)));
    } else {
        add(WAVE_TILE[bwd][d32][a.qkv_dtype != 0][njt - 1], pairs, 64 * nw, bwd ? lds_bytes(Bwd16Lds(njt, a.dk, Lqp)) : lds_bytes(Fwd16Lds(njt, a.dk, nw)));
    }
    return true;
}

}  // namespace ortk

