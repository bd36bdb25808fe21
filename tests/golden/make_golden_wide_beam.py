#!/usr/bin/env python3
"""Golden fixture G15: the reference's beam search at widths 10, 12, 16 and 32 (CaptionModel.batch_beam_search through
mode="sample", sparse_caption/models/caption_model.py:56-226) on the tiny G1 model, 4 images per case.
    python tests/golden/make_golden_wide_beam.py      # writes tests/golden/g15_wide_beam.npz
Per case: seq, logprobs, p of the reference, the input seed, and min_gap of tests/beam_ref.py (which must reproduce the
reference's tokens).  The cases and the share of images that must be comparable (min_gap >= GAP) are beam_ref.CASES; a seed that
misses its condition is replaced by the next one upwards that meets it, and the seed taken is stored."""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root (oracle/)
import common as C  # noqa: E402
from make_golden import import_reference, load_weights, tt  # noqa: E402


def main():
    import torch
    torch.manual_seed(0)
    torch.set_num_threads(4)
    get_model, Config, _, _, _ = import_reference()
    import beam_ref as R
    import helpers as H
    from oracle import ort_oracle as O
    model = get_model("relation_transformer")(Config(**C.TINY_CFG))
    load_weights(model, C.G1_SEED, C.G1_GEN_SCALE, C.G1_EOS_BIAS)
    model.eval()
    P = H.g1_state()
    cfg = O.OCfg(**{k: v for k, v in C.TINY_CFG.items() if not k.startswith("prune")})
    g = {}
    for name, (b, opts, seed0, need) in R.CASES.items():
        for seed in range(seed0, seed0 + 200):
            batch = R.case_inputs(C, seed)
            tb = tt(batch, ("att_feats", "boxes", "att_masks"))
            with torch.no_grad():
                seq, lp, p, gap = R.beam_search(P, cfg, tb["att_feats"], tb["boxes"], tb["att_masks"], b, **opts)
            if int((gap >= R.GAP).sum()) >= need:
                break
            print(f"{name}: seed {seed} leaves {int((gap >= R.GAP).sum())} of {R.N_IMG} images comparable, {need} needed")
        else:
            raise SystemExit(f"{name}: no seed in {seed0} .. {seed0 + 199} meets the condition")
        with torch.no_grad():
            seq_r, lp_r = model(att_feats=tb["att_feats"], boxes=tb["boxes"], att_masks=tb["att_masks"], opt=dict(opts, beam_size=b), mode="sample")
        p_r = np.array([[d["p"] for d in db] for db in model.done_beams], np.float32)
        assert torch.equal(seq_r, seq), f"{name}: beam_ref and the reference decode different tokens"
        assert int((gap >= R.GAP).sum()) >= need
        print(name, "seed", seed, "min_gap", gap.tolist(), "max |lp - ref|", float((lp_r - lp).abs().max()),
              "max |p - ref|", float(np.abs(p_r - p.numpy()).max()))
        g[f"{name}/seed"] = np.int64(seed)
        g[f"{name}/seq"] = seq_r.numpy()
        g[f"{name}/logprobs"] = lp_r.numpy()
        g[f"{name}/p"] = p_r
        g[f"{name}/min_gap"] = gap.numpy()
    C.save_golden(os.path.join(HERE, "g15_wide_beam.npz"), g)


if __name__ == "__main__":
    main()
