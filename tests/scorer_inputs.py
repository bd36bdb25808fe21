"""Seeded inputs shared by the reference-pack scorer tests (CPU host walk and GPU kernel): golden G6 in token-id space and
a randomised batch of references / hypothesis rows with the conditions the comparison relies on."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PAD, EOS = 0, 3
WEIGHTS = ((1.0, None), (0.5, [0.1, 0.2, 0.3, 0.4]))


def g6():
    return json.load(open(os.path.join(HERE, "golden", "g6_scst_scorer.json")))


def g6_id_space(g, L=24):
    """Golden G6 in token-id space, as tests/test_scorer_host.py::test_score_sequences_lives_in_the_df_table_space builds it:
    ids 4.. in reverse alphabetical order.  Returns (id_table, ref_ids, sample (N, ns, L), greedy (N, 1, L))."""
    table = {tuple(k): v for k, v in g["df"]}
    words = sorted({w for img in g["refs"] + g["sample"] + g["baseline"] for c in img for w in c.split()} | {w for k in table for w in k})
    w2i = {w: 4 + i for i, w in enumerate(reversed(words))}
    enc = lambda sent: ([w2i[w] for w in sent.split()][:L - 1] + [EOS] + [PAD] * L)[:L]
    assert all(len(c.split()) < L for img in g["sample"] + g["baseline"] for c in img)
    sample = np.array([[enc(c) for c in img] for img in g["sample"]], dtype=np.int64)
    greedy = np.array([[enc(img[0])] for img in g["baseline"]], dtype=np.int64)
    ref_ids = [[[w2i[w] for w in c.split()] for c in img] for img in g["refs"]]
    id_table = {"document_frequency": {tuple(w2i[w] for w in k): v for k, v in table.items()}, "ref_len": g["ref_len"]}
    return id_table, ref_ids, sample, greedy


def random_batch(seed, n_images=256, ns=5, L=18, pad_overwrite=True):
    """Per image 1-7 references of 5..L-1 tokens drawn from 60 ids; each hypothesis is a copy of one of its references with
    every token replaced with probability 0.3, then truncated at a random point (0.3), extended by 1-5 random tokens (0.2) or
    doubled (0.15), cut to L; 2 % of the hypotheses are empty (EOS first).  Rows shorter than L end in EOS then PAD; in 5 % of
    the rows one interior token is overwritten with PAD and the EOS removed (the scorer must cut there).
    Returns (refs, sample (N, ns, L), greedy (N, 1, L), caps) — caps[i][j] = the tokens row j of image i scores (j = ns: greedy)."""
    rs = np.random.RandomState(seed)
    tok = lambda size: rs.randint(4, 64, size=size)
    refs, rows, caps = [], [], []
    for _ in range(n_images):
        r = [[int(t) for t in tok(rs.randint(5, L))] for _ in range(rs.randint(1, 8))]
        refs.append(r)
        img_rows, img_caps = [], []
        for _ in range(ns + 1):
            h = np.array(r[rs.randint(len(r))])
            h = np.where(rs.uniform(size=h.size) < 0.3, tok(h.size), h)
            u = rs.uniform()
            if u < 0.3:
                h = h[:rs.randint(1, h.size + 1)]
            elif u < 0.5:
                h = np.concatenate([h, tok(rs.randint(1, 6))])
            elif u < 0.65:
                h = np.concatenate([h, h])
            h = h[:L]
            if rs.uniform() < 0.02:
                h = h[:0]
            row = np.full(L, PAD, dtype=np.int64)
            row[:h.size] = h
            if h.size < L:
                row[h.size] = EOS
            if pad_overwrite and rs.uniform() < 0.05 and h.size >= 3:
                cut = rs.randint(1, h.size - 1)
                row[cut] = PAD
                if h.size < L:
                    row[h.size] = PAD
                h = h[:cut]
            img_rows.append(row)
            img_caps.append([int(t) for t in h])
        rows.append(img_rows)
        caps.append(img_caps)
    rows = np.array(rows, dtype=np.int64)
    return refs, np.ascontiguousarray(rows[:, :ns]), np.ascontiguousarray(rows[:, ns:]), caps


def random_table(refs, seed):
    """A document-frequency table in token-id space for the cached mode: the n-grams of the batch's references with seeded
    counts (a part of them left out, so that some hypothesis n-grams miss the table), ref_len 5000."""
    rs = np.random.RandomState(seed + 1000)
    grams = sorted({tuple(c[i:i + k]) for r in refs for c in r for k in range(1, 5) for i in range(len(c) - k + 1)})
    keep = rs.uniform(size=len(grams)) < 0.9
    counts = rs.randint(1, 400, size=len(grams))
    return {"document_frequency": {g: float(c) for g, c, kp in zip(grams, counts, keep) if kp}, "ref_len": 5000.0}


def host_scores(table, refs, sample, greedy, wc, wb, baseline):
    """(sc_sample, sc_baseline) of the HOST scorer (CaptionScorer.score_sequences -> ortk_scorer_score)."""
    from sparse_image_captioning_amd.scst import CaptionScorer
    sc = CaptionScorer(table, cider_weight=wc, bleu_weight=wb)
    return sc.score_sequences(refs, sample, greedy if baseline == "greedy" else None, eos_idx=EOS, pad_idx=PAD)


def assert_input_conditions(table, refs, sample, greedy, caps, L):
    """Asserted on the HOST scorer's output before any comparison, so that the comparison cannot pass on rows that score
    nothing: >= 90 % of the hypotheses have CIDEr-D > 0, >= 40 % BLEU-4 > 1e-3, at least one is empty, >= 5 % are exactly L tokens."""
    from sparse_image_captioning_amd.scst import CaptionScorer
    N, ns = sample.shape[:2]
    both = np.concatenate([sample, greedy], 1).reshape(N * (ns + 1), 1, L)      # every row as a "sample" of its own image
    refs_rep = [r for r in refs for _ in range(ns + 1)]
    # (cached table: a row's score does not depend on the rest of the batch)
    dummy = np.zeros((both.shape[0], 1, L), dtype=np.int64)
    cider, _ = CaptionScorer(table, cider_weight=1.0).score_sequences(refs_rep, both, dummy, eos_idx=EOS, pad_idx=PAD)
    bleu4, _ = CaptionScorer(table, cider_weight=0.0, bleu_weight=[0.0, 0.0, 0.0, 1.0]).score_sequences(refs_rep, both, dummy, eos_idx=EOS, pad_idx=PAD)
    lens = np.array([len(c) for img in caps for c in img])
    stats = dict(cider_pos=float((cider > 0).mean()), bleu4_pos=float((bleu4 > 1e-3).mean()), empty=int((lens == 0).sum()),
                 full=float((lens == L).mean()))
    print("input conditions:", stats)
    assert stats["cider_pos"] >= 0.90 and stats["bleu4_pos"] >= 0.40 and stats["empty"] >= 1 and stats["full"] >= 0.05, stats
    return stats
