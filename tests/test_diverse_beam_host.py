"""Diverse beam search (group_size > 1), CPU side: tests/diverse_beam_ref.py reproduces the repaired reference's groups of golden
G16 (tests/golden/make_golden_diverse_beam.py) and their recorded decision margins, reduces to tests/beam_ref.py where it must
(lambda 0: every group; one group: the whole search), and the option parsing refuses what the library refuses — no device."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import beam_ref as R
import common as C
import diverse_beam_ref as D
import helpers as H
from oracle import ort_oracle as O


def _cfg():
    return O.OCfg(**{k: v for k, v in C.TINY_CFG.items() if not k.startswith("prune")})


_RUNS = {}


def _restated(golden, case):
    """the restatement on the case's stored inputs, computed once"""
    if case not in _RUNS:
        b, G, opts, _, _ = D.CASES[case]
        cb = H.torch_batch(D.case_inputs(C, int(golden("g16_diverse_beam")[f"{case}/seed"])))
        with torch.no_grad():
            _RUNS[case] = (cb, D.diverse_beam_search(H.g1_state(), _cfg(), cb["att_feats"], cb["boxes"], cb["att_masks"], b, G, **opts))
    return _RUNS[case]


@pytest.mark.parametrize("case", list(D.CASES))
def test_restatement_reproduces_the_golden_and_its_margins(golden, case):
    g = golden("g16_diverse_beam")
    assert int(g[f"{case}/seed"]) >= D.CASES[case][3]
    seq, lp, p, gap = _restated(golden, case)[1]
    np.testing.assert_array_equal(seq.numpy(), g[f"{case}/seq"])
    np.testing.assert_array_equal(gap.numpy(), g[f"{case}/min_gap"])
    np.testing.assert_allclose(lp.numpy(), g[f"{case}/logprobs"], rtol=0, atol=2e-5)      # (the bars of tests/test_beam_wide_host.py for G15)
    np.testing.assert_allclose(p.numpy(), g[f"{case}/p"], rtol=0, atol=5e-5)


def test_golden_meets_the_conditions_of_its_cases(golden):
    g = golden("g16_diverse_beam")
    for case, (b, G, opts, seed0, need) in D.CASES.items():
        gap, seq, p, lp = g[f"{case}/min_gap"], g[f"{case}/seq"], g[f"{case}/p"], g[f"{case}/logprobs"]
        bd = b // G
        assert seq.shape == (D.N_IMG, b, C.TINY_CFG["max_seq_length"]) and p.shape == (D.N_IMG, b) and lp.shape == seq.shape
        assert int((gap >= D.GAP).sum()) >= need, (case, gap.tolist())
        pg = p.reshape(D.N_IMG, G, bd)
        assert (np.diff(pg, axis=2) <= 0).all(), case                       # every group's list is sorted by score
        for img in seq.reshape(D.N_IMG, G, bd, -1):
            assert all(len({tuple(r) for r in grp.tolist()}) == bd for grp in img), case      # distinct captions inside a group


@pytest.mark.parametrize("case", ["b6_g2_l0"])
def test_lambda_zero_groups_equal_the_plain_beam_search(golden, case):
    """Without a penalty every group is the plain beam search of width bd (bit for bit: the same operations on the same tensors)."""
    b, G, opts, _, _ = D.CASES[case]
    bd = b // G
    cb, (seq, lp, p, gap) = _restated(golden, case)
    with torch.no_grad():
        ps, pl, pp, pgap = R.beam_search(H.g1_state(), _cfg(), cb["att_feats"], cb["boxes"], cb["att_masks"], bd)
    for g in range(G):
        rows = slice(g * bd, (g + 1) * bd)
        assert torch.equal(seq[:, rows], ps) and torch.equal(lp[:, rows], pl) and torch.equal(p[:, rows], pp), g
    assert torch.equal(gap, pgap)


@pytest.mark.parametrize("case", ["b4_g2", "b8_g2_wu_dc"])
def test_group_zero_is_the_plain_beam_search(golden, case):
    b, G, opts, _, _ = D.CASES[case]
    bd = b // G
    cb, (seq, lp, p, _) = _restated(golden, case)
    with torch.no_grad():
        ps, pl, pp, _ = R.beam_search(H.g1_state(), _cfg(), cb["att_feats"], cb["boxes"], cb["att_masks"], bd,
                                      **{k: v for k, v in opts.items() if k != "diversity_lambda"})
    assert torch.equal(seq[:, :bd], ps) and torch.equal(lp[:, :bd], pl) and torch.equal(p[:, :bd], pp)
    assert not torch.equal(seq[:, bd:2 * bd], ps)                           # ... and the penalty moves group 1


@pytest.mark.parametrize("b,opts", [(5, {}), (3, {"length_penalty": "wu_0.7", "decoding_constraint": 1, "diversity_lambda": 0.8})])
def test_one_group_equals_beam_ref(b, opts):
    P, cb = H.g1_state(), H.g1_batch()
    with torch.no_grad():
        want = R.beam_search(P, _cfg(), cb["att_feats"], cb["boxes"], cb["att_masks"], b, **{k: v for k, v in opts.items() if k != "diversity_lambda"})
        got = D.diverse_beam_search(P, _cfg(), cb["att_feats"], cb["boxes"], cb["att_masks"], b, 1, **opts)
    for w, g in zip(want, got):
        assert torch.equal(w, g)


# ------------------------------------------------------------------------------------------------ options
def _model(**over):
    import sparse_image_captioning_amd as P
    from sparse_image_captioning_amd.utils.config import Config
    return P.get_model("relation_transformer")(Config(**dict(C.TINY_CFG, **over)))


def test_decode_opts_parse_groups():
    m = _model()
    o, K, ex = m._decode_opts({"beam_size": 6, "seed": 1})
    assert (o.group_size, K) == (1, 6) and o.diversity_lambda == 0.5            # the reference's defaults (caption_model.py:117-118)
    o, K, ex = m._decode_opts({"beam_size": 6, "group_size": 3, "diversity_lambda": 0.8, "seed": 1})
    assert (o.group_size, K, ex) == (3, 6, "auto") and o.diversity_lambda == float(np.float32(0.8))
    assert not (o.exec_flags & (2 | 4 | 8 | 16 | 64 | 128))                     # no executor of the stack family
    o, K, _ = m._decode_opts({"beam_size": 4, "group_size": 4, "diversity_lambda": 0, "executor": "unfused", "seed": 1})
    assert (o.group_size, K, o.diversity_lambda) == (4, 4, 0.0)                 # one beam per group
    # one group: the plain decode whatever lambda is
    o, _, _ = m._decode_opts({"beam_size": 3, "group_size": 1, "diversity_lambda": -1.0, "seed": 1})
    assert o.group_size == 1
    o, _, _ = m._decode_opts({"num_random_sample": 3, "beam_size": 0, "group_size": 1, "seed": 1})
    assert o.group_size == 1
    for opt, why in (({"beam_size": 6, "group_size": 4}, "not a multiple of group_size=4"),
                     ({"beam_size": 3, "group_size": 6}, "exceeds beam_size=3"),
                     ({"beam_size": 4, "group_size": 0}, "expected an integer >= 1"),
                     ({"beam_size": 4, "group_size": -2}, "expected an integer >= 1"),
                     ({"beam_size": 4, "group_size": 2, "diversity_lambda": -0.5}, "finite number >= 0"),
                     ({"beam_size": 4, "group_size": 2, "diversity_lambda": float("nan")}, "finite number >= 0"),
                     ({"beam_size": 4, "group_size": 2, "diversity_lambda": float("inf")}, "finite number >= 0"),
                     ({"beam_size": 4, "group_size": 2, "diversity_lambda": 1e39}, "finite number >= 0"),
                     ({"beam_size": 0, "num_random_sample": 4, "group_size": 2}, "beam decodes"),
                     ({"beam_size": 66, "group_size": 2}, "ORTK_MAX_BEAM"),
                     ({"beam_size": 4, "group_size": 2, "executor": "stack"}, 'executor="stack" does not serve group_size=2'),
                     ({"beam_size": 4, "group_size": 2, "executor": "stack_split"}, "does not serve group_size"),
                     ({"beam_size": 4, "group_size": 2, "executor": "sparse_stream"}, "does not serve group_size"),
                     ({"beam_size": 4, "group_size": 2, "executor": "stack_fp8"}, "does not serve group_size")):
        with pytest.raises(ValueError, match=why):
            m._decode_opts(dict(opt, seed=1))


def test_decode_workspace_bytes_counts_the_groups_and_refuses_what_decode_refuses():
    import sparse_image_captioning_amd as P
    L = P._lib
    lib = L.lib()
    m = _model()

    def nbytes(**kw):
        o = L.DecodeOpts()
        o.beam_size, o.temperature, o.diversity_lambda = 6, 1.0, 0.5
        for k, v in kw.items():
            setattr(o, k, v)
        return lib.ortk_decode_workspace_bytes(Ct.byref(m._ccfg), 4, 9, Ct.byref(o))

    plain = nbytes()
    assert plain > 0 and nbytes(group_size=1) == plain and nbytes(group_size=1, diversity_lambda=-3.0) == plain
    # the same rows, and per-group finished counters and one group's output rows on top
    for G in (2, 3, 6):
        assert plain < nbytes(group_size=G) < plain + (1 << 16), G
    assert nbytes(group_size=2, exec_flags=L.DEC_UNFUSED) == nbytes(group_size=2) == nbytes(group_size=2, exec_flags=L.DEC_SPLIT_SMALL)
    assert nbytes(group_size=32, beam_size=32) > 0
    for kw in ({"group_size": 4}, {"group_size": 12}, {"group_size": -1}, {"group_size": 2, "diversity_lambda": -0.1},
               {"group_size": 2, "diversity_lambda": float("nan")}, {"group_size": 2, "diversity_lambda": float("inf")},
               {"group_size": 2, "beam_size": 0, "num_random_sample": 4}, {"group_size": 2, "beam_size": 66},
               {"group_size": 2, "exec_flags": L.DEC_STACK}, {"group_size": 2, "exec_flags": L.DEC_SPARSE_STREAM},
               {"group_size": 2, "exec_flags": L.DEC_STACK | L.DEC_STACK_SPLIT}, {"group_size": 2, "exec_flags": L.DEC_STACK | L.DEC_STACK_FP8},
               {"group_size": 2, "exec_flags": L.DEC_STACK | L.DEC_STACK_RB20}):
        assert nbytes(**kw) == 0, kw
    B, S = 4, 9
    assert m.decode_supported(B, S, {"beam_size": 6, "group_size": 3})
    assert m.decode_supported(B, S, {"beam_size": 6, "group_size": 3, "executor": "unfused"})
    for opt in ({"beam_size": 6, "group_size": 4}, {"beam_size": 6, "group_size": 3, "executor": "stack"},
                {"beam_size": 6, "group_size": 3, "diversity_lambda": -1.0}, {"beam_size": 0, "num_random_sample": 2, "group_size": 2}):
        assert not m.decode_supported(B, S, opt), opt
