// ortk_scorer_dev.hip — SCST reward scorer on the DEVICE: CIDEr-D and BLEU-1..4 of the sampled token rows against a
// reference pack cooked on the host (ortk_scorer.hip: ortk_scorer_pack_refs), one kernel on the caller's stream.
//
// One workgroup per image, one wavefront per hypothesis row (8 waves; an image with more rows takes another round).  The
// image's reference block (a few KB: 5 references x <= 66 keys x 20 B) is staged into LDS once and shared by its rows; a
// block above the staging buffer is read in place.  A row of L tokens has at most 4 L - 6 n-gram slots, lane l owns slots
// l, l + 64, ... (<= 4 of them at L = 64, kept in registers): duplicate counting and "first occurrence" are lane-against-LDS
// compares, the document-frequency lookup is one hash probe per slot, a reference lookup one binary search per slot, and
// every sum over the slots is a fixed-order xor butterfly.  fp64 throughout, as on the host (the scoring core is shared with
// the host walk: ortk_scorer_core.h).  No atomics and nothing that depends on scheduling: two runs give identical bits.
#include "ortk_common.h"
#include "ortk_scorer_core.h"

namespace {
namespace sc = ortk_sc;

constexpr int WAVES = 8;
constexpr int SLOTS_PER_LANE = (sc::MAX_SLOTS + ORTK_WAVE - 1) / ORTK_WAVE;      // 4
constexpr int STAGE_BYTES = 40 * 1024;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, ORTK_WAVE);      // (a + b == b + a: every lane ends with the same bits)
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, ORTK_WAVE);
    return v;
}

__global__ __launch_bounds__(WAVES * ORTK_WAVE) void scorer_pack_kernel(const ortk_scorer_pack_args a) {
    __shared__ __attribute__((aligned(16))) unsigned char s_blk[STAGE_BYTES];
    __shared__ uint64_t s_key[WAVES][SLOTS_PER_LANE * ORTK_WAVE];
    __shared__ int32_t s_tok[WAVES][sc::MAX_L];
    __shared__ double s_score[sc::MAX_ROWS];

    const int img = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ns = a.ns, rows = ns + (a.greedy ? 1 : 0), n = a.n, L = a.L;
    const unsigned char* pack = (const unsigned char*)a.pack;
    const sc::PackHdr* ph = (const sc::PackHdr*)pack;
    if (ph->magic != sc::PACK_MAGIC || ph->version != sc::PACK_VERSION || ph->n_images != a.n_images) {
        // not a pack of this batch: nothing of it is read; the outputs are poisoned so that the update cannot pass silently
        for (int j = tid; j < ns; j += WAVES * ORTK_WAVE) {
            const int64_t o = (int64_t)img * ns + j;
            a.reward[o] = __builtin_nanf("");
            if (a.score_sample) a.score_sample[o] = __builtin_nan("");
            if (a.score_baseline) a.score_baseline[o] = __builtin_nan("");
        }
        return;
    }
    const unsigned char* blk = pack + sc::pack_img_off(pack)[img];
    const int blk_bytes = sc::img_hdr(blk)->bytes;
    if (blk_bytes <= STAGE_BYTES) {      // (uniform over the workgroup)
        const uint64_t* src = (const uint64_t*)blk;
        uint64_t* dst = (uint64_t*)s_blk;
        for (int i = tid; i < blk_bytes / 8; i += WAVES * ORTK_WAVE) dst[i] = src[i];
        __syncthreads();
        blk = s_blk;
    }
    const sc::RefHdr* rf = sc::img_refs(blk);
    const uint64_t* rkey = sc::img_keys(blk);
    const double* rvec = sc::img_vec(blk);
    const int32_t* rcnt = sc::img_cnt(blk);
    const int nref = sc::img_hdr(blk)->nref;
    const unsigned char* dft = (const unsigned char*)a.df_table;
    const bool use_c = a.cider_weight > 0.0, use_b = sc::use_bleu(a.bleu_weight);

    for (int base = 0; base < rows; base += WAVES) {      // (uniform trip count: the barriers below are reached by every wave)
        const int row = base + wave;
        const bool active = row < rows;
        int len = 0, total = 0;
        if (active) {
            const int64_t* tok = row < ns ? a.sample + ((int64_t)img * ns + row) * a.sample_stride : a.greedy + (int64_t)img * a.greedy_stride;
            const int64_t t = lane < L ? tok[lane] : (int64_t)a.pad;
            const uint64_t stop = __ballot(t == (int64_t)a.eos || t == (int64_t)a.pad);      // lanes >= L carry PAD: a full row is cut at L
            len = stop ? __ffsll((unsigned long long)stop) - 1 : L;
            s_tok[wave][lane] = (int32_t)t;
            total = sc::slot_total(len);
        }
        __syncthreads();
        uint64_t key[SLOTS_PER_LANE];
        int ord[SLOTS_PER_LANE], sbeg[SLOTS_PER_LANE], send[SLOTS_PER_LANE];
#pragma unroll
        for (int p = 0; p < SLOTS_PER_LANE; ++p) {
            const int s = lane + p * ORTK_WAVE;
            key[p] = 0; ord[p] = 0; sbeg[p] = 0; send[p] = 0;
            if (s < total) {
                int k, i;
                sc::slot_pos(len, s, k, i, sbeg[p], send[p]);
                key[p] = sc::pack_key(&s_tok[wave][i], k);
                ord[p] = k - 1;
                s_key[wave][s] = key[p];
            }
        }
        __syncthreads();
        if (active) {
            int cnt[SLOTS_PER_LANE], mx[SLOTS_PER_LANE];
            double hv[SLOTS_PER_LANE];
            double nsq[sc::MAXN] = {0, 0, 0, 0};
#pragma unroll
            for (int p = 0; p < SLOTS_PER_LANE; ++p) {
                const int s = lane + p * ORTK_WAVE;
                cnt[p] = 0; mx[p] = 0; hv[p] = 0.0;
                if (s < total) {
                    cnt[p] = sc::slot_count(s_key[wave], s, sbeg[p], send[p]);
                    if (use_c && cnt[p] > 0 && ord[p] < n) hv[p] = sc::tfidf(cnt[p], sc::df_lookup(dft, key[p]), a.ref_len_log);
                }
#pragma unroll
                for (int o = 0; o < sc::MAXN; ++o) nsq[o] += ord[p] == o ? hv[p] * hv[p] : 0.0;
            }
            double hnorm[sc::MAXN], cscore[sc::MAXN] = {0, 0, 0, 0};
#pragma unroll
            for (int o = 0; o < sc::MAXN; ++o) hnorm[o] = use_c ? sqrt(wave_sum_f64(nsq[o])) : 0.0;
            const int hlength = sc::hyp_length(len, n);
            for (int r = 0; r < nref; ++r) {
                double val[sc::MAXN] = {0, 0, 0, 0};
#pragma unroll
                for (int p = 0; p < SLOTS_PER_LANE; ++p) {
                    if (cnt[p] == 0) continue;
                    const int q = sc::ref_find(rkey, rf[r], key[p]);
                    if (q < 0) continue;
                    mx[p] = max(mx[p], (int)rcnt[q]);
                    const double vr = rvec[q], term = fmin(hv[p], vr) * vr;
#pragma unroll
                    for (int o = 0; o < sc::MAXN; ++o) val[o] += (ord[p] == o && o < n) ? term : 0.0;
                }
                if (use_c) {
#pragma unroll
                    for (int o = 0; o < sc::MAXN; ++o)
                        if (o < n) cscore[o] += sc::cider_ref_term(wave_sum_f64(val[o]), hnorm[o], rf[r].norm[o], hlength, rf[r].length, a.sigma);
                }
            }
            const double cider = use_c ? sc::cider_finish(cscore, n, nref) : 0.0;
            double bleu[4] = {0, 0, 0, 0};
            if (use_b) {
                int correct[4];
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    int c = 0;
#pragma unroll
                    for (int p = 0; p < SLOTS_PER_LANE; ++p) c += (cnt[p] > 0 && ord[p] == o) ? min(mx[p], cnt[p]) : 0;
                    correct[o] = wave_sum_i32(c);
                }
                sc::bleu_finish(correct, len, sc::closest_reflen(blk, len), bleu);
            }
            if (lane == 0) s_score[row] = sc::combine(cider, bleu, a.cider_weight, a.bleu_weight);
        }
    }
    __syncthreads();
    for (int j = tid; j < ns; j += WAVES * ORTK_WAVE) {
        const double base = sc::baseline_score(s_score, ns, j, a.baseline, a.greedy ? s_score[ns] : 0.0);
        const int64_t o = (int64_t)img * ns + j;
        a.reward[o] = (float)(s_score[j] - base);
        if (a.score_sample) a.score_sample[o] = s_score[j];
        if (a.score_baseline) a.score_baseline[o] = base;
    }
}

}  // namespace

extern "C" int ortk_scorer_score_pack_device(const ortk_scorer_pack_args* a, void* stream) {
    if (!sc::args_ok(a)) return -1;
    hipLaunchKernelGGL(scorer_pack_kernel, dim3((unsigned)a->n_images), dim3(WAVES * ORTK_WAVE), 0, (hipStream_t)stream, *a);
    ORTK_CHECK_LAUNCH();
    return 0;
}
