// ortk_decode_joint.hip — the joint diverse executor's kernels (ORTK_DEC_GROUPS_JOINT, ortk.h): the selection steps of all groups of a
// global step in one launch, and the per-row arrays of a joint decoder pass.  A translation unit of its own, so that the kernels of
// ortk_decode.hip compile to what they were.
#include <algorithm>
#include "ortk_beam_dev.h"

namespace ortk {
namespace {

// The grouped steps of ALL groups of one global step Tg in one launch (the joint diverse executor, ortk.h: ORTK_DEC_GROUPS_JOINT): one
// workgroup per image walks the groups in ascending order and does, for every group with a local step t = Tg - g in 0 .. L - 1, what
// beam_step_diverse_kernel does for it — the same three device functions on the group's own state, which is st0 moved by g group
// strides.  Group g's penalty list reads the histories the groups p < g of the SAME image re-ordered earlier in this launch: writer
// and reader are this workgroup, and the __syncthreads() that ends every group's turn (a workgroup barrier with workgroup-scope
// release / acquire) orders them; nothing crosses workgroups.  The loop is bounded by G <= ORTK_MAX_BEAM.
template <int NPT, bool FASTEXP = false, bool STATS = false>
__global__ __launch_bounds__(256) void beam_step_diverse_joint_kernel(BeamState st0, JointGroups jg, int Tg, float scale_later, float lambda) {
    __shared__ WideLds S;
    __shared__ PenLds Pn;
    __shared__ int end_slot[WMAXB];
    // the group's state lives in LDS: beam_commit indexes its ping-pong pointers by the step's parity, which on a per-thread copy of
    // the kernel argument means scratch memory (328 bytes per lane when first built so)
    __shared__ __attribute__((aligned(16))) unsigned char st_raw[sizeof(BeamState)];
    BeamState& st = *reinterpret_cast<BeamState*>(st_raw);
    const int b = st0.b, L = st0.L, tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * b;
    for (int g = 0; g < jg.G; ++g) {
        const int t = Tg - g;
        if (t < 0 || t > L - 1) continue;                               // (the same for every thread: not started, or finished)
        const int64_t r = (int64_t)g * jg.rows;                          // rows before this group's block
        if (tid == 0) {      // (no thread still reads the previous group's state: the barrier that ended its turn)
            BeamState n = st0;
            n.seq[0] += r * L; n.seq[1] += r * L; n.tok_lp[0] += r * L; n.tok_lp[1] += r * L;
            n.kvidx[0] += r * (L + 1); n.kvidx[1] += r * (L + 1);
            n.cum += r; n.it += r; n.done_seq += r * L * L; n.done_lp += r * L * L; n.done_p += r * L; n.done_len += r * L;
            n.done_cnt += (int64_t)g * st0.B;
            n.gstats = STATS ? (t == 0 ? jg.gstats0 : jg.gstats + r * st0.nblk * 2) : nullptr;
            st = n;
        }
        __syncthreads();
        // position 0 reads the B-row pass of its own; later positions the group's block of the joint pass
        const float* logp = t == 0 ? jg.logp0 : jg.logp + r * st0.ldv;
        const float scale = t == 0 ? 1.f : scale_later;
        const int nq = t == 0 ? 1 : b;
        const int cur = t & 1;
        const int64_t srow0 = t == 0 ? (int64_t)blockIdx.x : row0;
        const int n_pen = g * b;
        int raw = -1;
        if (tid < n_pen) {
            const int p = tid / b, q = tid - p * b;
            const int steps = min(t + g - p, L - 1) + 1;                // local steps group p has done
            raw = ((steps & 1) ? st0.seq[1] : st0.seq[0])[(int64_t)p * jg.rows * L + (row0 + q) * L + t];
        }
        pen_build(Pn, raw, n_pen, lambda);
        beam_select_wide<true, NPT, FASTEXP, STATS, true>(S, logp + srow0 * st.ldv, st.ldv, nq, b, st.V, scale, t == 0 ? nullptr : st.cum + row0,
                                                          (st.decoding_constraint && t > 0) ? st.seq[cur] + row0 * L + t - 1 : nullptr, L,
                                                          STATS ? st.gstats + srow0 * st.nblk * 2 : nullptr, st.nblk, &Pn);
        beam_commit(st, logp, t, scale, S.win_v, S.win_i, S.row_mx, S.row_lse, end_slot);
        // the joint pass addresses ONE cache over all groups: a new beam's own slot is numbered from the first group's first row
        // (beam_commit numbered it inside the group's block; the same thread wrote it)
        if (tid < b) st.kvidx[cur ^ 1][(row0 + tid) * (t + 2) + t + 1] = (int32_t)((r + row0 + tid) * st0.tmax + t + 1);
        __syncthreads();          // this group's histories are written, S / Pn / end_slot are free: the next group's turn
    }
}

// the per-row arrays of the joint pass of global step Tg: row i of block g = i / rows is at position t = Tg - g if 1 <= t <= L - 1
// (key count t + 1, its ancestry entries at row stride t + 1 in the table of parity t & 1, kv_pp elements apart), otherwise idle:
// position 0, no keys.  tok_tab (G * rows, L): the row's token at its position, the layout embed_fwd_rows reads through row_pos.
__global__ void joint_rows_kernel(const int64_t* __restrict__ it, int64_t* __restrict__ tok_tab, int32_t* __restrict__ row_pos,
                                  int32_t* __restrict__ lk_row, int64_t* __restrict__ kv_off, int64_t rows, int G, int L, int Tg, int64_t kv_pp) {
    const int64_t n = rows * G;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t g = i / rows, rl = i - g * rows;
        const int t = Tg - (int)g;
        const bool active = t >= 1 && t <= L - 1;
        const int pos = active ? t : 0;
        tok_tab[i * L + pos] = it[i];
        row_pos[i] = (int32_t)(i * L + pos);
        lk_row[i] = active ? t + 1 : 0;
        kv_off[i] = active ? (int64_t)(t & 1) * kv_pp + g * rows * (L + 1) + rl * (t + 1) : 0;
    }
}
// ancestry tables of the joint executor before a group's position 0: image i of block g keeps its one row in the first slot of its
// first beam's cache rows, numbered over all groups' caches
__global__ void joint_kvidx_init_kernel(int32_t* __restrict__ kvidx, int64_t rows, int B, int b, int G, int L) {
    const int64_t n = (int64_t)B * G;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t g = i / B, img = i - g * B;
        kvidx[g * rows * (L + 1) + img] = (int32_t)((g * rows + img * b) * L);
    }
}

inline unsigned ew_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ortk_cdiv(n, 256), 2048)); }
}  // namespace

int beam_step_diverse_joint(const BeamState& st0, const JointGroups& jg, int32_t Tg, hipStream_t s, float scale_later, bool fast_exp, float lambda) {
    if (st0.b < 1 || jg.G < 1 || (int64_t)jg.G * st0.b > ORTK_MAX_BEAM || Tg < 0 || !(lambda >= 0.f) || lambda == INFINITY) return ORTK_EINVAL;
    if (jg.rows != (int64_t)st0.B * st0.b || !jg.logp || !jg.logp0) return ORTK_EINVAL;
    if (st0.B == 0) return 0;
    // the instance <NPT, FASTEXP, STATS> beam_step_diverse picks in the same mode (statistics only at temperature 1: position 0 and the
    // later positions then agree on the scale 1)
    const bool stats = fast_exp && jg.gstats && jg.gstats0 && scale_later == 1.f && st0.nblk <= 256 && st0.nblk * 64 >= st0.V, reg_rows = st0.V <= 256 * 40;
#define ORTK_BEAM_STEP(...) hipLaunchKernelGGL((beam_step_diverse_joint_kernel<__VA_ARGS__>), dim3((unsigned)st0.B), dim3(256), 0, s, st0, jg, Tg, scale_later, lambda)
    if (stats) ORTK_BEAM_STEP(0, true, true);
    else if (reg_rows && fast_exp) ORTK_BEAM_STEP(40, true);
    else if (reg_rows) ORTK_BEAM_STEP(40);
    else ORTK_BEAM_STEP(0);
#undef ORTK_BEAM_STEP
    ORTK_CHECK_LAUNCH();
    return 0;
}
int joint_rows(const int64_t* it, int64_t* tok_tab, int32_t* row_pos, int32_t* lk_row, int64_t* kv_off, int64_t rows, int32_t G, int32_t L, int32_t Tg,
               int64_t kv_pp, hipStream_t s) {
    if (rows < 0 || G < 1 || L < 1 || rows * G * L > 0x7FFFFFFF) return ORTK_EINVAL;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(joint_rows_kernel, dim3(ew_grid(rows * G)), dim3(256), 0, s, it, tok_tab, row_pos, lk_row, kv_off, rows, (int)G, (int)L, (int)Tg, kv_pp);
    ORTK_CHECK_LAUNCH();
    return 0;
}
int joint_kvidx_init(int32_t* kvidx, int64_t rows, int32_t B, int32_t b, int32_t G, int32_t L, hipStream_t s) {
    if (B == 0) return 0;
    hipLaunchKernelGGL(joint_kvidx_init_kernel, dim3(ew_grid((int64_t)B * G)), dim3(256), 0, s, kvidx, rows, (int)B, (int)b, (int)G, (int)L);
    ORTK_CHECK_LAUNCH();
    return 0;
}
}  // namespace ortk
