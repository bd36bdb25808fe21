"""fp64 restatement of truncated sampling (include/ortk.h: ortk_decode_opts.top_k / top_p, ortk_sample_truncate), i.e. of the
"top<k>" / "top<p>" branches of the reference's CaptionModel.sample_next_word (caption_model.py:246-266), for the tests.

One row at a time.  Candidates: every column but `banned`.  Total order: larger value first, the lower column on equal values.  The
kept set is a prefix of that order:
  top-k    the first min(k, candidates) entries;
  nucleus  with p_v = softmax(z / temperature) over the candidates, entry j is kept iff the mass strictly before it is < top_p
           (caption_model.py:254-256: `mask = cumsum < top_num`, shifted right by one with a leading one) — at least one entry.
"""
import numpy as np


def parse_method(method):
    """"top<k>" / "top<p>" -> (top_k, top_p), as the reference parses it: float(method[3:]), 0 < x < 1 means nucleus."""
    x = float(method[3:])
    return (0, x) if 0 < x < 1 else (int(x), 0.0)


def order(z, banned=-1):
    """Candidate columns of row `z`, best first."""
    z = np.asarray(z, np.float64)
    cols = np.arange(z.size)
    cols = cols[cols != banned]
    return cols[np.lexsort((cols, -z[cols]))]


def probs(z, temperature, cols):
    """softmax(z / temperature) over `cols` in fp64."""
    x = np.asarray(z, np.float64)[cols] / float(temperature)
    e = np.exp(x - x.max())
    return e / e.sum()


def kept(z, temperature=1.0, top_k=0, top_p=0.0, banned=-1):
    """-> dict(order, probs (in that order), n: entries kept, before: fp64 mass strictly before every entry of the order)."""
    assert (top_k > 0) != (top_p > 0)
    o = order(z, banned)
    if o.size == 0:
        return dict(order=o, probs=np.zeros(0), n=0, before=np.zeros(0))
    p = probs(z, temperature, o)
    before = np.concatenate([[0.0], np.cumsum(p)[:-1]])
    n = min(int(top_k), o.size) if top_k > 0 else max(1, int((before < top_p).sum()))
    return dict(order=o, probs=p, n=n, before=before)


def kept_mask(z, temperature=1.0, top_k=0, top_p=0.0, banned=-1):
    """Boolean mask over the columns of row `z`."""
    r = kept(z, temperature, top_k, top_p, banned)
    m = np.zeros(np.asarray(z).size, bool)
    m[r["order"][:r["n"]]] = True
    return m


def mask_from_cut(z, thr, thr_col, banned=-1):
    """The kept set an (thr, thr_col) pair of ortk_sample_truncate describes: z > thr, or z == thr and column <= thr_col, minus the
    banned column."""
    z = np.asarray(z)
    cols = np.arange(z.size)
    return ((z > thr) | ((z == thr) & (cols <= thr_col))) & (cols != banned)
