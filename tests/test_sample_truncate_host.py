"""Truncated sampling (top-k / nucleus), CPU side: the fp64 restatement the GPU tests compare with reproduces the kept sets of the
reference's own CaptionModel.sample_next_word (golden G14); `opt["sample_method"]` is parsed as the reference parses it and every
refusal names its reason; ortk_decode_workspace_bytes refuses what ortk.h lists (host arithmetic, no device)."""
import ctypes as C

import numpy as np
import pytest

import common as Cm
import sample_ref as R

CASES = ("top3", "top5", "top0.8", "top0.5")


def test_sample_ref_reproduces_the_reference_kept_sets(golden):
    g = golden("g14_sample_truncate")
    logp = g["logprobs"]
    assert logp.shape == (16, 101) and logp.dtype == np.float32
    for method in CASES:
        T = float(g[f"{method}/temperature"])
        want = np.unpackbits(g[f"{method}/keep_bits"])[:logp.size].reshape(logp.shape).astype(bool)
        k, p = R.parse_method(method)
        got = np.stack([R.kept_mask(row, T, k, p) for row in logp])
        assert np.array_equal(got, want), method
        # the (thr, thr_col) description of a kept set, as ortk_sample_truncate reports it, selects the same columns
        for row, keep in zip(logp, want):
            r = R.kept(row, T, k, p)
            last = r["order"][r["n"] - 1]
            assert np.array_equal(R.mask_from_cut(row, row[last], last), keep)
    assert [float(g[f"{m}/temperature"]) for m in CASES] == [1.0, np.float32(0.9), 1.0, np.float32(1.3)]


def test_sample_ref_ties_banned_and_edges():
    z = np.array([1.0, 2.0, 2.0, 0.5, 2.0, 1.0], np.float32)
    assert R.order(z).tolist() == [1, 2, 4, 0, 5, 3]                        # equal values: the lower column first
    assert R.kept_mask(z, top_k=2).tolist() == [False, True, True, False, False, False]
    assert R.kept_mask(z, top_k=2, banned=1).tolist() == [False, False, True, False, True, False]      # the banned column does not count
    assert R.kept_mask(z, top_k=99, banned=3).sum() == 5
    assert R.kept_mask(z, top_p=1e-9).tolist() == [False, True, False, False, False, False]            # at least one entry
    p = R.probs(z, 1.0, R.order(z))
    # an entry is kept iff the mass strictly before it is < top_p: a prefix that reaches top_p exactly is not extended
    assert R.kept(z, top_p=float(p[0] + p[1]))["n"] == 2 and R.kept(z, top_p=float(p[0] + p[1]) * (1 + 1e-12))["n"] == 3
    assert R.kept(np.zeros(1, np.float32), top_k=1, banned=0)["n"] == 0


def _model(**over):
    import sparse_image_captioning_amd as P
    from sparse_image_captioning_amd.utils.config import Config
    return P.get_model("relation_transformer")(Config(**dict(Cm.TINY_CFG, **over)))


def test_decode_opts_parse_sample_method():
    m = _model()
    base = {"num_random_sample": 3, "beam_size": 0, "seed": 1}
    for method, want in ((None, (0, 0.0)), ("sample", (0, 0.0)), ("top1", (1, 0.0)), ("top5", (5, 0.0)), ("top20000", (20000, 0.0)),
                         ("top3.0", (3, 0.0)), ("top0.8", (0, 0.8)), ("top0.05", (0, 0.05)), ("top1e-3", (0, 1e-3))):
        opt = dict(base) if method is None else dict(base, sample_method=method)
        o, K, _ = m._decode_opts(opt)
        assert (o.top_k, K) == (want[0], 3) and abs(o.top_p - want[1]) < 1e-7, method
        assert R.parse_method(method) == want if method not in (None, "sample") else True
    # plain decodes carry no truncation
    o, _, _ = m._decode_opts({"beam_size": 3})
    assert (o.top_k, o.top_p) == (0, 0.0)
    for bad, why in (("top", "not a number"), ("topk", "not a number"), ("top0", "integer k >= 1"), ("top-2", "integer k >= 1"),
                     ("top2.5", "integer k >= 1"), ("top1.0000001", "integer k >= 1"), ("topnan", "integer k >= 1"),
                     ("gumbel", 'expected "sample"'), ("greedy", 'expected "sample"'), ("Top5", 'expected "sample"'), (5, 'expected "sample"')):
        with pytest.raises(ValueError, match=why):
            m._decode_opts(dict(base, sample_method=bad))
    # a truncating method needs sampling rows
    for opt in ({"beam_size": 1}, {"beam_size": 3}, {"num_random_sample": 0, "beam_size": 1}):
        with pytest.raises(ValueError, match="num_random_sample > 0"):
            m._decode_opts(dict(opt, sample_method="top5", seed=1))
    # ... and a vocabulary the kernel holds in registers
    big = _model(vocab_size=10241)
    with pytest.raises(ValueError, match="at most 10240 tokens, this model has 10241"):
        big._decode_opts(dict(base, sample_method="top0.9"))
    big._decode_opts(dict(base))                         # (plain sampling of that model is served)
    _model(vocab_size=10240)._decode_opts(dict(base, sample_method="top0.9"))


def test_decode_workspace_bytes_refuses_bad_truncation():
    import sparse_image_captioning_amd as P
    L = P._lib
    lib = L.lib()
    m, big = _model(), _model(vocab_size=10241)

    def nbytes(mod, **kw):
        o = L.DecodeOpts()
        o.beam_size, o.num_random_sample, o.temperature = 0, 3, 1.0
        for k, v in kw.items():
            setattr(o, k, v)
        return lib.ortk_decode_workspace_bytes(C.byref(mod._ccfg), 4, 9, C.byref(o))

    plain = nbytes(m)
    assert plain > 0
    # served; the workspace is that of the plain decode (the logit rows exist in it already)
    for kw in ({"top_k": 1}, {"top_k": 5}, {"top_k": 20000}, {"top_p": 0.5}, {"top_p": 1e-6}, {"top_p": float(np.float32(1 - 2.0 ** -24))},
               {"top_k": 5, "with_greedy": 1}, {"top_p": 0.9, "decoding_constraint": 1}, {"top_k": 5, "exec_flags": L.DEC_UNFUSED}):
        assert nbytes(m, **kw) == nbytes(m, **{k: v for k, v in kw.items() if k not in ("top_k", "top_p")}) > 0, kw
    # refused
    for kw in ({"top_k": 5, "top_p": 0.5}, {"top_k": -1}, {"top_p": -0.1}, {"top_p": 1.0}, {"top_p": 1.5}, {"top_p": float("nan")},
               {"top_k": 5, "num_random_sample": 0, "beam_size": 1}, {"top_p": 0.5, "num_random_sample": 0, "beam_size": 3}):
        assert nbytes(m, **kw) == 0, kw
    assert nbytes(big) > 0 and nbytes(big, top_k=5) == 0 and nbytes(big, top_p=0.5) == 0
    assert nbytes(_model(vocab_size=10240), top_k=5) > 0
