// ortk_scorer_core.h — the scoring logic and the reference-pack format shared by the HOST walk of a pack
// (ortk_scorer.hip: ortk_scorer_score_pack_host) and the DEVICE kernel (ortk_scorer_dev.hip: scorer_pack_kernel).
//
// Everything here is `__host__ __device__` and free of state: one hypothesis n-gram ("slot") at a time, so that the host
// walks the slots of a row in a loop and the device gives each lane of a wavefront its slots.  What differs between the two
// callers is only how the per-slot terms are summed (serial on the host, fixed-order butterfly on the device).
//
// Semantics, operation for operation in double precision (see ortk_scorer.hip for the reference lines):
//   CIDEr-D   vec = cnt * (ref_len_log - log(max(1, df))); per reference sum(min(vec_h, vec_r) * vec_r) / (|h| |r|) when both
//             norms are non-zero; Gaussian penalty on the bigram-count lengths; mean over orders and references; x 10
//   BLEU-1..4 counts clipped by the maximum reference count, closest reference length (ties to the shorter), tiny / small,
//             brevity penalty, cumulative geometric means
//
// ---- pack format (flat, position independent: every offset is relative to the start of the buffer; 8-byte aligned) ----
//   PackHdr                                   48 bytes
//   int64   img_off[n_images]                 byte offset of each image block
//   image block i:
//     ImgHdr                                  16 bytes
//     RefHdr  ref[nref]                       48 bytes each: first, nkeys, len, length (sum of bigram counts), norm[4]
//     uint64  key[nkeys]                      n-gram keys of orders 1..4; the range [first, first + nkeys) of reference r is
//                                             SORTED ascending (a lane finds a key by binary search; orders come out grouped,
//                                             a k-gram key is >= 2^(16 (k - 1)))
//     double  vec[nkeys]                      tf-idf value of the key (0 for orders above the scorer's n)
//     int32   cnt[nkeys] (+ pad to 8 bytes)   count of the key in the reference caption
// ---- document-frequency table (flat open addressing, linear probing, load <= 1/2) ----
//   DfHdr { nslots (power of two, 0 = empty table), nkeys }      16 bytes
//   DfSlot { key, df } [nslots]               key 0 = free slot (a packed n-gram is never 0: every field is id + 1)
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/ortk_scorer.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ORTK_SC_HD __host__ __device__ static inline
#else
#define ORTK_SC_HD static inline
#endif

namespace ortk_sc {

constexpr int MAXN = 4;
constexpr int MAX_L = 64;                        // longest row (check_cfg's max_seq_length limit)
constexpr int MAX_SLOTS = 4 * MAX_L - 6;         // n-gram positions of orders 1..4 in a row of MAX_L tokens (250)
constexpr int MAX_ROWS = 64;                     // hypothesis rows per image (samples + greedy)
constexpr uint32_t PACK_MAGIC = 0x4B50434Fu;     // "OCPK"
constexpr uint32_t PACK_VERSION = 1;
constexpr int BASELINE_GREEDY = ORTK_SCORER_BASELINE_GREEDY, BASELINE_LEAVE_ONE_OUT = ORTK_SCORER_BASELINE_LEAVE_ONE_OUT;

struct PackHdr {
    uint32_t magic, version;
    int32_t n_images, items_per_image;
    int32_t n, cached;
    int64_t bytes;
    double ref_len_log;
    int64_t reserved;
};
struct ImgHdr { int32_t nref, nkeys, bytes, pad; };
struct RefHdr { int32_t first, nkeys, len, length; double norm[MAXN]; };
struct DfHdr { uint64_t nslots, nkeys; };
struct DfSlot { uint64_t key; double df; };

static_assert(sizeof(PackHdr) == 48 && sizeof(ImgHdr) == 16 && sizeof(RefHdr) == 48 && sizeof(DfSlot) == 16, "pack layout");

ORTK_SC_HD int64_t align8(int64_t v) { return (v + 7) & ~(int64_t)7; }
ORTK_SC_HD int64_t img_block_bytes(int nref, int nkeys) {
    return (int64_t)sizeof(ImgHdr) + (int64_t)nref * (int64_t)sizeof(RefHdr) + (int64_t)nkeys * 16 + align8((int64_t)nkeys * 4);
}
ORTK_SC_HD const int64_t* pack_img_off(const unsigned char* pack) { return (const int64_t*)(pack + sizeof(PackHdr)); }
ORTK_SC_HD const ImgHdr* img_hdr(const unsigned char* blk) { return (const ImgHdr*)blk; }
ORTK_SC_HD const RefHdr* img_refs(const unsigned char* blk) { return (const RefHdr*)(blk + sizeof(ImgHdr)); }
ORTK_SC_HD const uint64_t* img_keys(const unsigned char* blk) {
    return (const uint64_t*)(blk + sizeof(ImgHdr) + (size_t)img_hdr(blk)->nref * sizeof(RefHdr));
}
ORTK_SC_HD const double* img_vec(const unsigned char* blk) { return (const double*)(img_keys(blk) + img_hdr(blk)->nkeys); }
ORTK_SC_HD const int32_t* img_cnt(const unsigned char* blk) { return (const int32_t*)(img_vec(blk) + img_hdr(blk)->nkeys); }

// ---- n-gram keys ----
ORTK_SC_HD uint64_t pack_key(const int32_t* w, int k) {
    uint64_t v = 0;
    for (int i = 0; i < k; ++i) v = (v << 16) | (uint64_t)(uint32_t)(w[i] + 1);
    return v;
}
ORTK_SC_HD int key_order(uint64_t key) { return (key >> 48) ? 3 : (key >> 32) ? 2 : (key >> 16) ? 1 : 0; }

// ---- document frequencies ----
ORTK_SC_HD uint64_t df_hash(uint64_t key, uint64_t mask) {
    key *= 0x9E3779B97F4A7C15ull;
    key ^= key >> 29;
    return key & mask;
}
ORTK_SC_HD double df_lookup(const unsigned char* table, uint64_t key) {
    if (!table) return 0.0;
    const uint64_t nslots = ((const DfHdr*)table)->nslots;
    if (nslots == 0) return 0.0;
    const DfSlot* slot = (const DfSlot*)(table + sizeof(DfHdr));
    const uint64_t mask = nslots - 1;
    uint64_t i = df_hash(key, mask);
    for (uint64_t probes = 0; probes < nslots; ++probes, i = (i + 1) & mask) {      // (bounded: a damaged table cannot spin)
        const uint64_t k = slot[i].key;
        if (k == key) return slot[i].df;
        if (k == 0) break;
    }
    return 0.0;
}
ORTK_SC_HD double tfidf(int cnt, double df, double ref_len_log) {      // counts2vec, ciderD_scorer.py:146-150
    return (double)cnt * (ref_len_log - log(fmax(1.0, df)));
}

// what the host walk and the device entry point can check without reading the buffers
static inline bool args_ok(const ortk_scorer_pack_args* a) {
    if (!a || !a->pack || !a->sample || !a->reward) return false;
    if (a->n < 1 || a->n > MAXN || !(a->sigma > 0.0)) return false;
    if (a->n_images < 1 || a->ns < 1 || a->L < 1 || a->L > MAX_L || a->sample_stride < a->L) return false;
    if (a->greedy && a->greedy_stride < a->L) return false;
    if (a->ns + (a->greedy ? 1 : 0) > MAX_ROWS) return false;
    if (a->baseline == BASELINE_GREEDY) return a->greedy != nullptr;
    if (a->baseline == BASELINE_LEAVE_ONE_OUT) return a->ns >= 2;
    return false;
}

// ---- rows and slots ----
// `length` of a hypothesis of `len` tokens: the sum of its bigram counts, taken inside the loop over the first n orders
// (ciderD_scorer.py:152-153), so 0 when n = 1
ORTK_SC_HD int hyp_length(int len, int n) { return n >= 2 && len > 1 ? len - 1 : 0; }
// A row is cut at the first EOS or PAD (score_sequences.cut); without either it is L tokens.
ORTK_SC_HD int cut_len(const int64_t* row, int L, int64_t eos, int64_t pad) {
    int len = 0;
    while (len < L && row[len] != eos && row[len] != pad) ++len;
    return len;
}
ORTK_SC_HD int slot_total(int len) {
    int t = 0;
    for (int k = 1; k <= MAXN; ++k) t += len - k + 1 > 0 ? len - k + 1 : 0;
    return t;
}
// slot s of a row of `len` tokens: the n-gram of order k (1..4) at position i; [begin, end) = the slots of that order
ORTK_SC_HD void slot_pos(int len, int s, int& k, int& i, int& begin, int& end) {
    begin = 0;
    for (k = 1; k <= MAXN; ++k) {
        const int c = len - k + 1 > 0 ? len - k + 1 : 0;
        if (s < begin + c || k == MAXN) { i = s - begin; end = begin + c; return; }
        begin += c;
    }
}
// count of slot s's key in the row, or 0 when an earlier slot already carries that key (the n-gram is scored once, at its
// first occurrence: the reference's dict insertion)
ORTK_SC_HD int slot_count(const uint64_t* keys, int s, int begin, int end) {
    const uint64_t key = keys[s];
    int cnt = 0;
    for (int j = begin; j < end; ++j) {
        if (keys[j] == key) {
            if (j < s) return 0;
            ++cnt;
        }
    }
    return cnt;
}
// key in reference r of the image block: index into key / vec / cnt, or -1
ORTK_SC_HD int ref_find(const uint64_t* keys, const RefHdr& r, uint64_t key) {
    int lo = r.first, hi = r.first + r.nkeys;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint64_t k = keys[mid];
        if (k == key) return mid;
        if (k < key) lo = mid + 1; else hi = mid;
    }
    return -1;
}

// ---- CIDEr-D ----
// sim() for one reference and one order, after the sum over the hypothesis n-grams (ciderD_scorer.py:176-183)
ORTK_SC_HD double cider_ref_term(double val, double hnorm, double rnorm, int hlength, int rlength, double sigma) {
    const double delta = (double)(hlength - rlength);
    if (hnorm != 0.0 && rnorm != 0.0) val /= hnorm * rnorm;
    return val * pow(M_E, -(delta * delta) / (2.0 * sigma * sigma));
}
ORTK_SC_HD double cider_finish(const double* score, int n, int nref) {
    double sum = 0.0;
    for (int o = 0; o < n; ++o) sum += score[o];
    double avg = sum / (double)n;
    avg /= (double)nref;
    return avg * 10.0;
}

// ---- BLEU ----
ORTK_SC_HD int closest_reflen(const unsigned char* blk, int testlen) {      // min over (|l - testlen|, l), bleu_scorer.py:74-75
    const RefHdr* rf = img_refs(blk);
    int best_d = 1 << 30, reflen = 0;
    for (int r = 0; r < img_hdr(blk)->nref; ++r) {
        const int l = rf[r].len, dd = l > testlen ? l - testlen : testlen - l;
        if (dd < best_d || (dd == best_d && l < reflen)) { best_d = dd; reflen = l; }
    }
    return reflen;
}
ORTK_SC_HD void bleu_finish(const int* correct, int testlen, int reflen, double* out) {
    const double small = 1e-9, tiny = 1e-15;
    double bleu = 1.0;
    for (int k = 0; k < 4; ++k) {
        const int guess = testlen - k > 0 ? testlen - k : 0;
        bleu *= ((double)correct[k] + tiny) / ((double)guess + small);
        out[k] = pow(bleu, 1.0 / (double)(k + 1));
    }
    const double ratio = ((double)testlen + tiny) / ((double)reflen + small);
    if (ratio < 1.0) {
        const double bp = exp(1.0 - 1.0 / ratio);
        for (int k = 0; k < 4; ++k) out[k] *= bp;
    }
}

// ---- score and reward ----
// CaptionScorer.score_ids: scores = 0 + cider * wc, then + bleu[k] * w[k] in order; a metric whose weights are all 0 is skipped
ORTK_SC_HD bool use_bleu(const double* wb) { return fmax(fmax(wb[0], wb[1]), fmax(wb[2], wb[3])) > 0.0; }
ORTK_SC_HD double combine(double cider, const double* bleu, double wc, const double* wb) {
    double s = 0.0;
    if (wc > 0.0) s = s + cider * wc;
    if (use_bleu(wb)) for (int k = 0; k < 4; ++k) s = s + bleu[k] * wb[k];
    return s;
}
// baseline score of sample j of an image whose `ns` sample scores are sc[0..ns): the greedy row's score, or the mean of the others
ORTK_SC_HD double baseline_score(const double* sc, int ns, int j, int kind, double greedy_score) {
    if (kind == BASELINE_GREEDY) return greedy_score;
    double sum = 0.0;
    for (int q = 0; q < ns; ++q) sum += sc[q];
    return (sum - sc[j]) / (double)(ns - 1);
}

}  // namespace ortk_sc
