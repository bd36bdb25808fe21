/* ortk_scorer.h — C-ABI of the SCST reward scorer: a HOST scorer (multi-threaded; no GPU involved) and a DEVICE scorer
 * (one HIP kernel on the caller's stream) that reads the sampled token tensor where the decode left it and writes the reward
 * where the SCST update reads it.  The device scorer splits the work by what it depends on: everything that depends on the
 * REFERENCES only is cooked on the host ahead of time into a flat "reference pack" (ortk_scorer_pack_refs: CPU code, no device
 * needed, usable in data-loader workers); everything that depends on the SAMPLED captions runs in the kernel.
  *
 * Replaces, on integer token sequences, the pure-Python reward computation that follows sampling in the reference's
 * self-critical step (sparse_caption/utils/training.py:239-252):
 *   CaptionScorer.__call__                         scst/scorers.py:47-107
 *   CiderD / CiderScorer (CIDEr-D, n = 4, sigma 6)  scst/cider/pyciderevalcap/ciderD/ciderD_scorer.py:18-226
 *   Bleu / BleuScorer per-sentence BLEU-1..4       coco_caption/pycocoevalcap/bleu/bleu_scorer.py:24-261 ("closest" length)
 * Words are interned to int32 ids by the caller (sparse-image-captioning_amd/scst/scorers.py does it for strings), so an
 * n-gram is up to 4 ids < 65535 packed exactly into 64 bits: no hashing collisions, results equal the reference's.
 * All arithmetic is double precision in the reference's operation order.
 */
#ifndef ORTK_SCORER_H
#define ORTK_SCORER_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ortk_scorer ortk_scorer;

/* n = n-gram order of CIDEr-D (the reference uses 4; 1..4 supported), sigma = Gaussian length-penalty width (6.0). */
ortk_scorer* ortk_scorer_create(int32_t n, double sigma);
void ortk_scorer_destroy(ortk_scorer* s);

/* Cached document frequencies (the reference's `coco-train-words.p`: {"document_frequency": {ngram: count}, "ref_len": D}).
 * n-gram i = tokens[key_off[i] .. key_off[i+1]), 1..4 ids each; ref_len = D (the log is taken inside, ciderD_scorer.py:88).
 * Without this call the scorer runs in "corpus" mode: document frequencies and D come from the references of each
 * ortk_scorer_score call (ciderD_scorer.py:117-128,190-192,221-226).  Returns 0, or -1 on a bad argument. */
int ortk_scorer_set_df(ortk_scorer* s, const int32_t* tokens, const int64_t* key_off, const double* df, int64_t nkeys,
                       double ref_len);

/* Scores `nitems` (hypothesis, references) items.
 *   caption c          = cap_tok[cap_off[c] .. cap_off[c+1])                 (table of ncaps captions, hypotheses and references)
 *   hypothesis of item i = caption hyp_cap[i]
 *   references of item i = captions ref_cap[item_ref_off[i] .. item_ref_off[i+1])   (>= 1 each)
 * cider_out (nitems) and/or bleu_out (4 x nitems, row k = BLEU-(k+1)) may be NULL.  nthreads <= 0: hardware concurrency.
 * Returns 0, -1 on a bad argument (a token >= 65535, an item without references, ...). */
int ortk_scorer_score(const ortk_scorer* s, const int32_t* cap_tok, const int64_t* cap_off, int64_t ncaps,
                      const int64_t* hyp_cap, const int64_t* ref_cap, const int64_t* item_ref_off, int64_t nitems,
                      double* cider_out, double* bleu_out, int32_t nthreads);

/* ---------------------------------------------------------------------------------------------------------------------
 * Reference pack + device scorer
 *
 * Pack format (flat, position independent, 8-byte aligned; csrc/ortk_scorer_core.h holds the structs and the shared
 * host/device scoring core):
 *   header (48 B: magic, version, n_images, items_per_image, n, cached, bytes, ref_len_log) | int64 img_off[n_images] |
 *   per image: { nref, nkeys, bytes } | per reference { first, nkeys, len, length, norm[4] } | uint64 key[nkeys] |
 *   double vec[nkeys] | int32 cnt[nkeys]
 * i.e. per reference caption the packed 64-bit n-gram keys of orders 1..4, their counts, their tf-idf values, the four
 * norms, `length` (sum of bigram counts) and `len`.  The keys of ONE reference are sorted ascending: a device lane finds a
 * hypothesis n-gram in a reference by binary search.
 * Document-frequency table: { nslots (power of two), nkeys } | { uint64 key, double df } [nslots] — open addressing, linear
 * probing from (key * 0x9E3779B97F4A7C15 ^ >> 29) & (nslots - 1), key 0 = free slot, load factor <= 1/2.
 * ------------------------------------------------------------------------------------------------------------------- */

/* Packs the references of `n_images` images: reference caption c = cap_tok[cap_off[c] .. cap_off[c+1]), the references of
 * image i = captions img_ref_off[i] .. img_ref_off[i+1]) (>= 1 each).
 * need[0] / need[1] always receive the bytes of the pack / of the batch's document-frequency table.
 *   pack_out == NULL: size query only.
 *   cached mode (ortk_scorer_set_df was called): reference tf-idf values come from that table; need[1] = 0, df_out is unused
 *     (serialise the table ONCE per scorer with ortk_scorer_df_table).
 *   corpus mode: the call also writes the batch's table to df_out.  The reference makes one document per hypothesis ITEM, so
 *     an image scored with `items_per_image` hypotheses (ns, or ns + 1 with a greedy baseline) adds items_per_image to the df
 *     of each of its reference n-grams and ref_len = n_images * items_per_image; computed per image, not per item.
 * *ref_len_log_out (may be NULL) receives log(ref_len) of the mode in use.
 * Returns 0, -1 on a bad argument (a token >= 65535, an image without references, items_per_image < 1), -2 when pack_bytes
 * or df_bytes is too small. */
int ortk_scorer_pack_refs(const ortk_scorer* s, const int32_t* cap_tok, const int64_t* cap_off, const int64_t* img_ref_off,
                          int64_t n_images, int32_t items_per_image, void* pack_out, int64_t pack_bytes, void* df_out,
                          int64_t df_bytes, int64_t* need, double* ref_len_log_out);

/* Cached mode: the whole ortk_scorer_set_df table as a flat hash table (the hypothesis side needs the idf of EVERY n-gram,
 * matched or not, for its norm).  out == NULL: size query (*need).  Returns 0, -1 (corpus mode / bad argument), -2 (too small). */
int ortk_scorer_df_table(const ortk_scorer* s, void* out, int64_t out_bytes, int64_t* need);

#define ORTK_SCORER_BASELINE_GREEDY 0          /* reward = score(sample) - score(greedy row of the same image) */
#define ORTK_SCORER_BASELINE_LEAVE_ONE_OUT 1   /* reward = score - (sum over the image's samples - score) / (ns - 1) */

typedef struct ortk_scorer_pack_args {
    const void* pack;             /* reference pack */
    const void* df_table;         /* document-frequency table (NULL: every df is 0) */
    double ref_len_log;           /* as returned by ortk_scorer_pack_refs */
    double sigma;                 /* Gaussian length-penalty width (6.0) */
    const int64_t* sample;        /* (n_images * ns) rows of L int64 tokens, row r at sample + r * sample_stride */
    int64_t sample_stride;
    const int64_t* greedy;        /* (n_images) rows of L tokens, or NULL; required by the greedy baseline */
    int64_t greedy_stride;
    int32_t n;                    /* CIDEr-D uses n-gram orders 1..n (1..4); BLEU always four */
    int32_t baseline;             /* ORTK_SCORER_BASELINE_* */
    int32_t n_images, ns, L;      /* ns + (greedy != NULL) <= 64 rows per image, 1 <= L <= 64 */
    int32_t eos, pad;             /* a row is cut at the first EOS or PAD; a row without either is L tokens; an empty row scores 0 */
    int32_t reserved;
    double cider_weight;          /* score = cider_weight * CIDEr-D + sum_k bleu_weight[k] * BLEU-(k+1); a metric whose weights */
    double bleu_weight[4];        /* are all 0 is skipped */
    float* reward;                /* out (n_images * ns) */
    double* score_sample;         /* out (n_images * ns), may be NULL */
    double* score_baseline;       /* out (n_images * ns), may be NULL */
} ortk_scorer_pack_args;

/* Scores token rows against a pack on the HOST (every pointer is host memory): the same scoring core as the kernel, so the
 * logic and the pack format are checked on a machine without a GPU.  Returns 0, -1 on a bad argument (a token outside
 * 0..65534 included). */
int ortk_scorer_score_pack_host(const ortk_scorer_pack_args* a);

/* The same on the DEVICE: every pointer is device memory, one kernel on `stream` (a hipStream_t), no allocation, no
 * synchronisation, no global state, no atomics: two runs give bit-identical outputs.  One workgroup per image, one
 * wavefront per hypothesis row; fp64 throughout.  Token ids cannot be checked without a synchronisation: the caller
 * guarantees ids in 0..65534 (the Python layer refuses a vocabulary above 65534).  Returns 0, -1 on a bad argument, or a
 * positive hipError_t. */
int ortk_scorer_score_pack_device(const ortk_scorer_pack_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ORTK_SCORER_H */
