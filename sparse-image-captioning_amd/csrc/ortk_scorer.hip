// ortk_scorer.hip — SCST reward scorer on the HOST (no device code in this file; it is built into libortk.so with the
// rest of the C-ABI): CIDEr-D and per-sentence BLEU-1..4 over integer n-grams, multi-threaded over items.  The second half
// cooks the reference pack of the device scorer (ortk_scorer_dev.hip) and walks a pack on the host.
//
// Follows, operation for operation in double precision:
//   precook / cook_refs / cook_test / counts2vec / sim / compute_cider   ciderD_scorer.py:18-214
//   precook / cook_refs / cook_test / compute_score (per-sentence list)  bleu_scorer.py:24-90,202-243
// The reference keeps n-grams as tuples of words in Python dicts; iteration order there is insertion order (n-gram
// length major, then first occurrence), which the cooked captions here reproduce so that the floating-point sums run
// in the same order.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <thread>
#include <unordered_map>
#include <vector>
#include <cstring>
#include "../../include/ortk_scorer.h"
#include "ortk_scorer_core.h"

namespace {

constexpr int MAXN = 4;

struct Cooked {
    int len = 0;                          // number of words
    std::vector<uint64_t> key;            // packed n-gram, insertion order
    std::vector<int> cnt;
    std::vector<int8_t> ord;              // n-gram length - 1
    // CIDEr side (filled once the document frequencies are known)
    std::vector<double> vec;
    double norm[MAXN] = {0, 0, 0, 0};
    int length = 0;                       // sum of bigram counts (ciderD_scorer.py:152-153: `if n == 1`)
};

inline uint64_t pack(const int32_t* w, int k) {
    uint64_t v = 0;
    for (int i = 0; i < k; ++i) v = (v << 16) | (uint64_t)(w[i] + 1);
    return v;
}

bool cook(const int32_t* w, int len, int n, Cooked& c) {
    c.len = len;
    for (int i = 0; i < len; ++i) if (w[i] < 0 || w[i] >= 65535) return false;
    for (int k = 1; k <= n; ++k) {
        const size_t first = c.key.size();
        for (int i = 0; i + k <= len; ++i) {
            const uint64_t kk = pack(w + i, k);
            size_t j = first;
            for (; j < c.key.size(); ++j) if (c.key[j] == kk) break;
            if (j == c.key.size()) { c.key.push_back(kk); c.cnt.push_back(1); c.ord.push_back((int8_t)(k - 1)); }
            else ++c.cnt[j];
        }
    }
    return true;
}

template <typename F>
void parallel_for(int64_t n, int nthreads, F f) {
    if (n <= 0) return;
    int nt = nthreads > 0 ? nthreads : (int)std::thread::hardware_concurrency();
    nt = (int)std::max<int64_t>(1, std::min<int64_t>(nt, n));
    if (nt == 1) { for (int64_t i = 0; i < n; ++i) f(i); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t)
        th.emplace_back([=]() { for (int64_t i = t; i < n; i += nt) f(i); });
    for (auto& x : th) x.join();
}

}  // namespace

struct ortk_scorer {
    int n;
    double sigma;
    bool cached = false;
    double ref_len_log = 0.0;
    std::unordered_map<uint64_t, double> df;
};

extern "C" ortk_scorer* ortk_scorer_create(int32_t n, double sigma) {
    if (n < 1 || n > MAXN || !(sigma > 0.0)) return nullptr;
    ortk_scorer* s = new ortk_scorer();
    s->n = n; s->sigma = sigma;
    return s;
}
extern "C" void ortk_scorer_destroy(ortk_scorer* s) { delete s; }

extern "C" int ortk_scorer_set_df(ortk_scorer* s, const int32_t* tokens, const int64_t* key_off, const double* df, int64_t nkeys,
                                  double ref_len) {
    if (!s || nkeys < 0 || (nkeys > 0 && (!tokens || !key_off || !df)) || !(ref_len > 0.0)) return -1;
    s->df.clear();
    s->df.reserve((size_t)nkeys * 2);
    for (int64_t i = 0; i < nkeys; ++i) {
        const int64_t k = key_off[i + 1] - key_off[i];
        if (k < 1 || k > MAXN) return -1;
        for (int64_t j = key_off[i]; j < key_off[i + 1]; ++j) if (tokens[j] < 0 || tokens[j] >= 65535) return -1;
        s->df[pack(tokens + key_off[i], (int)k)] = df[i];
    }
    s->ref_len_log = std::log(ref_len);
    s->cached = true;
    return 0;
}

extern "C" int ortk_scorer_score(const ortk_scorer* s, const int32_t* cap_tok, const int64_t* cap_off, int64_t ncaps,
                                 const int64_t* hyp_cap, const int64_t* ref_cap, const int64_t* item_ref_off, int64_t nitems,
                                 double* cider_out, double* bleu_out, int32_t nthreads) {
    if (!s || !cap_off || !hyp_cap || !ref_cap || !item_ref_off || ncaps < 0 || nitems < 0) return -1;
    if (nitems == 0) return 0;
    for (int64_t i = 0; i < nitems; ++i) {
        if (hyp_cap[i] < 0 || hyp_cap[i] >= ncaps || item_ref_off[i + 1] <= item_ref_off[i]) return -1;
        for (int64_t r = item_ref_off[i]; r < item_ref_off[i + 1]; ++r) if (ref_cap[r] < 0 || ref_cap[r] >= ncaps) return -1;
    }
    const int n = s->n;
    std::vector<Cooked> caps((size_t)ncaps);
    std::vector<char> ok((size_t)ncaps, 1);
    // BLEU always uses 4-grams (BleuSilent(4), scorers.py:52); CIDEr uses the first n orders of the same cooked captions
    parallel_for(ncaps, nthreads, [&](int64_t c) {
        ok[c] = cook(cap_tok + cap_off[c], (int)(cap_off[c + 1] - cap_off[c]), MAXN, caps[c]) ? 1 : 0;
    });
    for (int64_t c = 0; c < ncaps; ++c) if (!ok[c]) return -1;

    if (cider_out) {
        // document frequencies: cached table, or "corpus" mode over this call's items (one document per item)
        std::unordered_map<uint64_t, double> local;
        const std::unordered_map<uint64_t, double>* df = &s->df;
        double ref_len_log = s->ref_len_log;
        if (!s->cached) {
            std::vector<uint64_t> seen;
            for (int64_t i = 0; i < nitems; ++i) {
                seen.clear();
                for (int64_t r = item_ref_off[i]; r < item_ref_off[i + 1]; ++r) {
                    const Cooked& c = caps[ref_cap[r]];
                    for (size_t j = 0; j < c.key.size(); ++j) if (c.ord[j] < n) seen.push_back(c.key[j]);
                }
                std::sort(seen.begin(), seen.end());
                seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
                for (uint64_t k : seen) local[k] += 1.0;
            }
            df = &local;
            ref_len_log = std::log((double)nitems);
        }
        // counts2vec (ciderD_scorer.py:131-155)
        parallel_for(ncaps, nthreads, [&](int64_t ci) {
            Cooked& c = caps[ci];
            c.vec.assign(c.key.size(), 0.0);
            double nsq[MAXN] = {0, 0, 0, 0};
            c.length = 0;
            for (size_t j = 0; j < c.key.size(); ++j) {
                const int o = c.ord[j];
                if (o >= n) continue;
                const auto it = df->find(c.key[j]);
                const double d = std::log(std::max(1.0, it == df->end() ? 0.0 : it->second));
                const double v = (double)c.cnt[j] * (ref_len_log - d);
                c.vec[j] = v;
                nsq[o] += std::pow(v, 2);
                if (o == 1) c.length += c.cnt[j];
            }
            for (int o = 0; o < MAXN; ++o) c.norm[o] = std::sqrt(nsq[o]);
        });
        const double sigma = s->sigma;
        parallel_for(nitems, nthreads, [&](int64_t i) {
            const Cooked& h = caps[hyp_cap[i]];
            double score[MAXN] = {0, 0, 0, 0};
            const int64_t nref = item_ref_off[i + 1] - item_ref_off[i];
            for (int64_t r = item_ref_off[i]; r < item_ref_off[i + 1]; ++r) {
                const Cooked& rf = caps[ref_cap[r]];
                const double delta = (double)(h.length - rf.length);
                double val[MAXN] = {0, 0, 0, 0};
                for (size_t j = 0; j < h.key.size(); ++j) {
                    const int o = h.ord[j];
                    if (o >= n) continue;
                    double vr = 0.0;
                    for (size_t q = 0; q < rf.key.size(); ++q) if (rf.key[q] == h.key[j]) { vr = rf.vec[q]; break; }
                    val[o] += std::min(h.vec[j], vr) * vr;          // clipping (ciderD_scorer.py:176)
                }
                for (int o = 0; o < n; ++o) {
                    if (h.norm[o] != 0.0 && rf.norm[o] != 0.0) val[o] /= h.norm[o] * rf.norm[o];
                    val[o] *= std::pow(M_E, -(delta * delta) / (2.0 * sigma * sigma));
                    score[o] += val[o];
                }
            }
            double sum = 0.0;
            for (int o = 0; o < n; ++o) sum += score[o];
            double avg = sum / (double)n;
            avg /= (double)nref;
            avg *= 10.0;
            cider_out[i] = avg;
        });
    }

    if (bleu_out) {
        const double small = 1e-9, tiny = 1e-15;
        parallel_for(nitems, nthreads, [&](int64_t i) {
            const Cooked& h = caps[hyp_cap[i]];
            const int testlen = h.len;
            // closest reference length: min over (|l - testlen|, l) (bleu_scorer.py:74-75)
            int best_d = 1 << 30, reflen = 0;
            for (int64_t r = item_ref_off[i]; r < item_ref_off[i + 1]; ++r) {
                const int l = caps[ref_cap[r]].len, dd = std::abs(l - testlen);
                if (dd < best_d || (dd == best_d && l < reflen)) { best_d = dd; reflen = l; }
            }
            int correct[4] = {0, 0, 0, 0};
            for (size_t j = 0; j < h.key.size(); ++j) {
                int mx = 0;
                for (int64_t r = item_ref_off[i]; r < item_ref_off[i + 1]; ++r) {
                    const Cooked& rf = caps[ref_cap[r]];
                    for (size_t q = 0; q < rf.key.size(); ++q) if (rf.key[q] == h.key[j]) { mx = std::max(mx, rf.cnt[q]); break; }
                }
                correct[h.ord[j]] += std::min(mx, h.cnt[j]);
            }
            double bleu = 1.0, out[4];
            for (int k = 0; k < 4; ++k) {
                const int guess = std::max(0, testlen - k);
                bleu *= ((double)correct[k] + tiny) / ((double)guess + small);
                out[k] = std::pow(bleu, 1.0 / (double)(k + 1));
            }
            const double ratio = ((double)testlen + tiny) / ((double)reflen + small);
            if (ratio < 1.0) for (int k = 0; k < 4; ++k) out[k] *= std::exp(1.0 - 1.0 / ratio);
            for (int k = 0; k < 4; ++k) bleu_out[(int64_t)k * nitems + i] = out[k];
        });
    }
    return 0;
}

// =====================================================================================================================
// Reference pack of the device scorer (format: ortk_scorer_core.h) and its host walk
// =====================================================================================================================
namespace {
namespace sc = ortk_sc;

int64_t df_table_bytes(size_t nkeys, uint64_t* nslots_out) {
    uint64_t nslots = 0;
    if (nkeys > 0) { nslots = 16; while (nslots < 2 * (uint64_t)nkeys) nslots <<= 1; }
    if (nslots_out) *nslots_out = nslots;
    return (int64_t)(sizeof(sc::DfHdr) + nslots * sizeof(sc::DfSlot));
}

// keys are inserted in ascending order, so the bytes of a table depend on its content only
void df_table_write(std::vector<std::pair<uint64_t, double>>& kv, unsigned char* out) {
    uint64_t nslots;
    const int64_t bytes = df_table_bytes(kv.size(), &nslots);
    std::memset(out, 0, (size_t)bytes);
    sc::DfHdr* h = (sc::DfHdr*)out;
    h->nslots = nslots; h->nkeys = kv.size();
    sc::DfSlot* slot = (sc::DfSlot*)(out + sizeof(sc::DfHdr));
    std::sort(kv.begin(), kv.end());
    for (const auto& e : kv) {
        uint64_t i = sc::df_hash(e.first, nslots - 1);
        while (slot[i].key != 0) i = (i + 1) & (nslots - 1);
        slot[i].key = e.first; slot[i].df = e.second;
    }
}

}  // namespace

extern "C" int ortk_scorer_pack_refs(const ortk_scorer* s, const int32_t* cap_tok, const int64_t* cap_off, const int64_t* img_ref_off,
                                     int64_t n_images, int32_t items_per_image, void* pack_out, int64_t pack_bytes, void* df_out,
                                     int64_t df_bytes, int64_t* need, double* ref_len_log_out) {
    if (!s || !cap_off || !img_ref_off || !need || n_images < 1 || n_images > INT32_MAX || items_per_image < 1) return -1;
    if (img_ref_off[0] < 0) return -1;
    for (int64_t i = 0; i < n_images; ++i) if (img_ref_off[i + 1] <= img_ref_off[i]) return -1;      // an image without references
    const int64_t c0 = img_ref_off[0], ncaps = img_ref_off[n_images] - c0;
    const int n = s->n;
    std::vector<Cooked> caps((size_t)ncaps);
    for (int64_t c = 0; c < ncaps; ++c) {
        const int64_t a = cap_off[c0 + c], b = cap_off[c0 + c + 1];
        if (b < a || b - a > INT32_MAX / 8 || (b > a && !cap_tok)) return -1;
        if (!cook(cap_tok + a, (int)(b - a), MAXN, caps[(size_t)c])) return -1;
    }
    // sizes
    int64_t bytes = (int64_t)sizeof(sc::PackHdr) + n_images * 8;
    for (int64_t i = 0; i < n_images; ++i) {
        int64_t nkeys = 0;
        for (int64_t c = img_ref_off[i] - c0; c < img_ref_off[i + 1] - c0; ++c) nkeys += (int64_t)caps[(size_t)c].key.size();
        if (nkeys > INT32_MAX / 32) return -1;
        bytes += sc::img_block_bytes((int)(img_ref_off[i + 1] - img_ref_off[i]), (int)nkeys);
    }
    // document frequencies: cached table, or the batch's own — one document per hypothesis item, so an image counts
    // items_per_image times (computed per image: the items of an image share one reference list)
    std::unordered_map<uint64_t, double> local;
    const std::unordered_map<uint64_t, double>* df = &s->df;
    double ref_len_log = s->ref_len_log;
    if (!s->cached) {
        std::vector<uint64_t> seen;
        for (int64_t i = 0; i < n_images; ++i) {
            seen.clear();
            for (int64_t c = img_ref_off[i] - c0; c < img_ref_off[i + 1] - c0; ++c) {
                const Cooked& k = caps[(size_t)c];
                for (size_t j = 0; j < k.key.size(); ++j) if (k.ord[j] < n) seen.push_back(k.key[j]);
            }
            std::sort(seen.begin(), seen.end());
            seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
            for (uint64_t k : seen) local[k] += (double)items_per_image;
        }
        df = &local;
        ref_len_log = std::log((double)n_images * (double)items_per_image);
    }
    need[0] = bytes;
    need[1] = s->cached ? 0 : df_table_bytes(local.size(), nullptr);
    if (ref_len_log_out) *ref_len_log_out = ref_len_log;
    if (!pack_out) return 0;
    if (pack_bytes < need[0] || (need[1] > 0 && (!df_out || df_bytes < need[1]))) return -2;

    unsigned char* out = (unsigned char*)pack_out;
    std::memset(out, 0, (size_t)bytes);
    sc::PackHdr* h = (sc::PackHdr*)out;
    h->magic = sc::PACK_MAGIC; h->version = sc::PACK_VERSION;
    h->n_images = (int32_t)n_images; h->items_per_image = items_per_image;
    h->n = n; h->cached = s->cached ? 1 : 0;
    h->bytes = bytes; h->ref_len_log = ref_len_log;
    int64_t* img_off = (int64_t*)(out + sizeof(sc::PackHdr));
    int64_t at = (int64_t)sizeof(sc::PackHdr) + n_images * 8;
    std::vector<int> order;
    for (int64_t i = 0; i < n_images; ++i) {
        const int nref = (int)(img_ref_off[i + 1] - img_ref_off[i]);
        int nkeys = 0;
        for (int r = 0; r < nref; ++r) nkeys += (int)caps[(size_t)(img_ref_off[i] - c0 + r)].key.size();
        img_off[i] = at;
        unsigned char* blk = out + at;
        sc::ImgHdr* ih = (sc::ImgHdr*)blk;
        ih->nref = nref; ih->nkeys = nkeys; ih->bytes = (int32_t)sc::img_block_bytes(nref, nkeys);
        sc::RefHdr* rh = (sc::RefHdr*)(blk + sizeof(sc::ImgHdr));
        uint64_t* key = (uint64_t*)(rh + nref);
        double* vec = (double*)(key + nkeys);
        int32_t* cnt = (int32_t*)(vec + nkeys);
        int first = 0;
        for (int r = 0; r < nref; ++r) {
            const Cooked& c = caps[(size_t)(img_ref_off[i] - c0 + r)];
            const int nk = (int)c.key.size();
            // counts2vec in the reference's insertion order (the norms are sums in that order), then stored sorted by key
            std::vector<double> v((size_t)nk, 0.0);
            double nsq[MAXN] = {0, 0, 0, 0};
            int length = 0;
            for (int j = 0; j < nk; ++j) {
                const int o = c.ord[j];
                if (o >= n) continue;
                const auto it = df->find(c.key[j]);
                v[j] = sc::tfidf(c.cnt[j], it == df->end() ? 0.0 : it->second, ref_len_log);
                nsq[o] += std::pow(v[j], 2);
                if (o == 1) length += c.cnt[j];
            }
            rh[r].first = first; rh[r].nkeys = nk; rh[r].len = c.len; rh[r].length = length;
            for (int o = 0; o < MAXN; ++o) rh[r].norm[o] = std::sqrt(nsq[o]);
            order.resize((size_t)nk);
            for (int j = 0; j < nk; ++j) order[j] = j;
            std::sort(order.begin(), order.end(), [&](int a, int b) { return c.key[a] < c.key[b]; });
            for (int j = 0; j < nk; ++j) {
                key[first + j] = c.key[order[j]]; vec[first + j] = v[order[j]]; cnt[first + j] = c.cnt[order[j]];
            }
            first += nk;
        }
        at += ih->bytes;
    }
    if (need[1] > 0) {
        std::vector<std::pair<uint64_t, double>> kv(local.begin(), local.end());
        df_table_write(kv, (unsigned char*)df_out);
    }
    return 0;
}

extern "C" int ortk_scorer_df_table(const ortk_scorer* s, void* out, int64_t out_bytes, int64_t* need) {
    if (!s || !need || !s->cached) return -1;
    *need = df_table_bytes(s->df.size(), nullptr);
    if (!out) return 0;
    if (out_bytes < *need) return -2;
    std::vector<std::pair<uint64_t, double>> kv(s->df.begin(), s->df.end());
    df_table_write(kv, (unsigned char*)out);
    return 0;
}

extern "C" int ortk_scorer_score_pack_host(const ortk_scorer_pack_args* a) {
    if (!sc::args_ok(a)) return -1;
    const unsigned char* pack = (const unsigned char*)a->pack;
    const sc::PackHdr* h = (const sc::PackHdr*)pack;
    if (h->magic != sc::PACK_MAGIC || h->version != sc::PACK_VERSION || h->n_images != a->n_images) return -1;
    const unsigned char* dft = (const unsigned char*)a->df_table;
    const int n = a->n, L = a->L, ns = a->ns, rows = ns + (a->greedy ? 1 : 0);
    const bool use_c = a->cider_weight > 0.0, use_b = sc::use_bleu(a->bleu_weight);
    for (int64_t r = 0; r < (int64_t)a->n_images * ns; ++r)
        for (int t = 0; t < L; ++t) { const int64_t w = a->sample[r * a->sample_stride + t]; if (w < 0 || w >= 65535) return -1; }
    if (a->greedy)
        for (int64_t r = 0; r < a->n_images; ++r)
            for (int t = 0; t < L; ++t) { const int64_t w = a->greedy[r * a->greedy_stride + t]; if (w < 0 || w >= 65535) return -1; }
    std::vector<double> score((size_t)rows);
    for (int img = 0; img < a->n_images; ++img) {
        const unsigned char* blk = pack + sc::pack_img_off(pack)[img];
        const sc::RefHdr* rf = sc::img_refs(blk);
        const uint64_t* rkey = sc::img_keys(blk);
        const double* rvec = sc::img_vec(blk);
        const int32_t* rcnt = sc::img_cnt(blk);
        const int nref = sc::img_hdr(blk)->nref;
        for (int row = 0; row < rows; ++row) {      // row ns = the greedy row
            const int64_t* tok64 = row < ns ? a->sample + ((int64_t)img * ns + row) * a->sample_stride : a->greedy + (int64_t)img * a->greedy_stride;
            const int len = sc::cut_len(tok64, L, a->eos, a->pad);
            int32_t tok[sc::MAX_L];
            for (int t = 0; t < len; ++t) tok[t] = (int32_t)tok64[t];
            const int total = sc::slot_total(len);
            uint64_t key[sc::MAX_SLOTS];
            int cnt[sc::MAX_SLOTS];
            double hvec[sc::MAX_SLOTS];
            for (int sidx = 0; sidx < total; ++sidx) {
                int k, i, b, e;
                sc::slot_pos(len, sidx, k, i, b, e);
                key[sidx] = sc::pack_key(tok + i, k);
            }
            double nsq[MAXN] = {0, 0, 0, 0};
            for (int sidx = 0; sidx < total; ++sidx) {
                int k, i, b, e;
                sc::slot_pos(len, sidx, k, i, b, e);
                cnt[sidx] = sc::slot_count(key, sidx, b, e);
                hvec[sidx] = 0.0;
                if (use_c && cnt[sidx] > 0 && k <= n) {
                    hvec[sidx] = sc::tfidf(cnt[sidx], sc::df_lookup(dft, key[sidx]), a->ref_len_log);
                    nsq[k - 1] += hvec[sidx] * hvec[sidx];
                }
            }
            const int hlength = sc::hyp_length(len, n);
            double hnorm[MAXN], cscore[MAXN] = {0, 0, 0, 0};
            for (int o = 0; o < MAXN; ++o) hnorm[o] = std::sqrt(nsq[o]);
            int mx[sc::MAX_SLOTS];
            for (int sidx = 0; sidx < total; ++sidx) mx[sidx] = 0;
            for (int r = 0; r < nref; ++r) {
                double val[MAXN] = {0, 0, 0, 0};
                for (int sidx = 0; sidx < total; ++sidx) {
                    if (cnt[sidx] == 0) continue;
                    const int q = sc::ref_find(rkey, rf[r], key[sidx]);
                    if (q < 0) continue;
                    mx[sidx] = std::max(mx[sidx], (int)rcnt[q]);
                    const int o = sc::key_order(key[sidx]);
                    if (o < n) val[o] += std::min(hvec[sidx], rvec[q]) * rvec[q];
                }
                if (use_c) for (int o = 0; o < n; ++o) cscore[o] += sc::cider_ref_term(val[o], hnorm[o], rf[r].norm[o], hlength, rf[r].length, a->sigma);
            }
            const double cider = use_c ? sc::cider_finish(cscore, n, nref) : 0.0;
            double bleu[4] = {0, 0, 0, 0};
            if (use_b) {
                int correct[4] = {0, 0, 0, 0};
                for (int sidx = 0; sidx < total; ++sidx)
                    if (cnt[sidx] > 0) correct[sc::key_order(key[sidx])] += std::min(mx[sidx], cnt[sidx]);
                sc::bleu_finish(correct, len, sc::closest_reflen(blk, len), bleu);
            }
            score[(size_t)row] = sc::combine(cider, bleu, a->cider_weight, a->bleu_weight);
        }
        for (int j = 0; j < ns; ++j) {
            const double base = sc::baseline_score(score.data(), ns, j, a->baseline, a->greedy ? score[(size_t)ns] : 0.0);
            const int64_t o = (int64_t)img * ns + j;
            a->reward[o] = (float)(score[(size_t)j] - base);
            if (a->score_sample) a->score_sample[o] = score[(size_t)j];
            if (a->score_baseline) a->score_baseline[o] = base;
        }
    }
    return 0;
}
