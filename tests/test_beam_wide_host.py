"""Wide beam search, CPU side: tests/beam_ref.py restates `oracle.beam_search` bit for bit, reproduces the reference's tokens of
golden G15 (widths 10, 12, 16, 32; tests/golden/make_golden_wide_beam.py) and their recorded decision margins."""
import numpy as np
import pytest
import torch

import beam_ref as R
import common as C
import helpers as H
from oracle import ort_oracle as O


def _cfg():
    return O.OCfg(**{k: v for k, v in C.TINY_CFG.items() if not k.startswith("prune")})


@pytest.mark.parametrize("b,opts", [(3, {}), (5, {}), (3, {"length_penalty": "wu_0.7", "decoding_constraint": 1})])
def test_beam_ref_equals_oracle_bit_for_bit(b, opts):
    P, cb = H.g1_state(), H.g1_batch()
    with torch.no_grad():
        want = O.beam_search(P, _cfg(), cb["att_feats"], cb["boxes"], cb["att_masks"], b, **opts)
        got = R.beam_search(P, _cfg(), cb["att_feats"], cb["boxes"], cb["att_masks"], b, **opts)
    for w, g in zip(want, got[:3]):
        assert torch.equal(w, g)
    assert got[3].shape == (cb["att_feats"].size(0),) and bool((got[3] >= 0).all())


@pytest.mark.parametrize("case", list(R.CASES))
def test_beam_ref_reproduces_the_golden_and_its_margins(golden, case):
    g = golden("g15_wide_beam")
    b, opts, seed0, need = R.CASES[case]
    seed = int(g[f"{case}/seed"])
    assert seed >= seed0
    cb = H.torch_batch(R.case_inputs(C, seed))
    with torch.no_grad():
        seq, lp, p, gap = R.beam_search(H.g1_state(), _cfg(), cb["att_feats"], cb["boxes"], cb["att_masks"], b, **opts)
    np.testing.assert_array_equal(seq.numpy(), g[f"{case}/seq"])
    np.testing.assert_array_equal(gap.numpy(), g[f"{case}/min_gap"])
    np.testing.assert_allclose(lp.numpy(), g[f"{case}/logprobs"], rtol=0, atol=2e-5)      # (reference vs oracle on a CPU: 3.7e-6)
    np.testing.assert_allclose(p.numpy(), g[f"{case}/p"], rtol=0, atol=5e-5)              # (1.1e-5)


def test_golden_meets_the_conditions_of_its_cases(golden):
    g = golden("g15_wide_beam")
    for case, (b, opts, seed0, need) in R.CASES.items():
        gap, seq, p, lp = g[f"{case}/min_gap"], g[f"{case}/seq"], g[f"{case}/p"], g[f"{case}/logprobs"]
        assert seq.shape == (R.N_IMG, b, C.TINY_CFG["max_seq_length"]) and p.shape == (R.N_IMG, b)
        assert int((gap >= R.GAP).sum()) >= need, (case, gap.tolist())
        assert (np.diff(p, axis=1) <= 0).all(), case
        assert all(len({tuple(r) for r in img.tolist()}) == b for img in seq), case
        if not opts.get("length_penalty"):
            np.testing.assert_allclose(lp.sum(-1), p, rtol=0, atol=2e-4)
