"""Edge schedules of the joint diverse executor (tests/test_gpu_diverse_joint.py, tests/test_diverse_joint_host.py): the smallest
shapes at which the window of active groups behaves differently, on the tiny model (18 positions) and the G1 input recipe.

case -> (b, G, decode options, input seed, images that must have min_gap >= GAP).  The seeds are the first, from 75 upwards, on which
the CPU restatement (tests/diverse_beam_ref.py) leaves at least half of the 4 images with a decision margin; what it measured there:
    b5_g5        min_gap 1.1e-02 7.6e-03 9.1e-04 1.6e-02
    b10_g2       min_gap 1.2e-03 1.4e-03 9.3e-04 7.4e-04
    b20_g20      min_gap 2.8e-03 9.4e-04 4.6e-04 1.4e-04      (one image below GAP = 2e-4)
    b9_g3_wu_dc  min_gap 4.2e-03 2.2e-03 1.9e-03 3.9e-03"""
import torch

import common as C
import diverse_beam_ref as D
import helpers as H
from oracle import ort_oracle as O

EDGE_CASES = {
    "b5_g5": (5, 5, {}, 75, 2),                    # one beam per group (bd = 1)
    "b10_g2": (10, 2, {}, 75, 2),                  # two groups: the window is full for all but two global steps
    "b20_g20": (20, 20, {}, 75, 2),                # more groups than positions: groups finish before others start
    "b9_g3_wu_dc": (9, 3, {"length_penalty": "wu_0.7", "decoding_constraint": 1, "diversity_lambda": 0.4}, 75, 2),
}

_RUNS = {}


def oracle_cfg(cfg=C.TINY_CFG):
    return O.OCfg(**{k: v for k, v in cfg.items() if not k.startswith("prune")})


def restated(case):
    """(inputs, (seq, logprobs, p, min_gap)) of the restatement on the case's inputs, computed once per process"""
    if case not in _RUNS:
        b, G, opts, seed, _ = EDGE_CASES[case]
        cb = H.torch_batch(D.case_inputs(C, seed))
        with torch.no_grad():
            _RUNS[case] = (cb, D.diverse_beam_search(H.g1_state(), oracle_cfg(), cb["att_feats"], cb["boxes"], cb["att_masks"], b, G, **opts))
    return _RUNS[case]
