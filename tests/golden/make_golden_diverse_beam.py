#!/usr/bin/env python3
"""Golden fixture G16: the reference's DIVERSE beam search (CaptionModel.batch_beam_search with group_size > 1 through
mode="sample", sparse_caption/models/caption_model.py:33-52, 151-218) on the tiny G1 model, 4 images per case.
    python tests/golden/make_golden_diverse_beam.py      # writes tests/golden/g16_diverse_beam.npz
The imported reference gets two repairs, attached at run time, without which its path does not run or is not the
algorithm it states:
  1. `repeat_tensor`, which caption_model.py:50 calls and no class defines: the row-wise repeat of the file's upstream;
  2. the position counter: PositionalEncoding.current_time_step counts calls of the module, and the groups take turns inside one
     time loop; after `_update_caches` installed a group's caches the counter is set to the number of cached self-attention keys,
     so that every group is embedded at its own position.
Per case: seq, logprobs, p of the repaired reference, the input seed, and min_gap of tests/diverse_beam_ref.py (which must decode
the reference's tokens).  The cases and the number of images that must be comparable (min_gap >= GAP) are diverse_beam_ref.CASES;
the first seed from the case's start upwards that meets the condition is taken and stored."""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root (oracle/)
import common as C  # noqa: E402
from make_golden import import_reference, load_weights, tt  # noqa: E402


def repair(model):
    import torch
    type(model).repeat_tensor = lambda self, n, x: torch.repeat_interleave(x, n, dim=0)
    inner = model._update_caches

    def update_caches(caches):
        inner(caches)
        pos = model.model.decoder.layers[0].self_attn.cache[0].size(2)
        for m in model.modules():
            if hasattr(m, "current_time_step"):
                m.current_time_step = pos

    model._update_caches = update_caches


def main():
    import torch
    torch.manual_seed(0)
    torch.set_num_threads(4)
    get_model, Config, _, _, _ = import_reference()
    import diverse_beam_ref as D
    import helpers as H
    from oracle import ort_oracle as O
    model = get_model("relation_transformer")(Config(**C.TINY_CFG))
    load_weights(model, C.G1_SEED, C.G1_GEN_SCALE, C.G1_EOS_BIAS)
    model.eval()
    repair(model)
    P = H.g1_state()
    cfg = O.OCfg(**{k: v for k, v in C.TINY_CFG.items() if not k.startswith("prune")})
    g = {}
    for name, (b, G, opts, seed0, need) in D.CASES.items():
        for seed in range(seed0, seed0 + 200):
            batch = D.case_inputs(C, seed)
            tb = tt(batch, ("att_feats", "boxes", "att_masks"))
            with torch.no_grad():
                seq, lp, p, gap = D.diverse_beam_search(P, cfg, tb["att_feats"], tb["boxes"], tb["att_masks"], b, G, **opts)
            if int((gap >= D.GAP).sum()) >= need:
                break
            print(f"{name}: seed {seed} leaves {int((gap >= D.GAP).sum())} of {D.N_IMG} images comparable, {need} needed")
        else:
            raise SystemExit(f"{name}: no seed in {seed0} .. {seed0 + 199} meets the condition")
        with torch.no_grad():
            seq_r, lp_r = model(att_feats=tb["att_feats"], boxes=tb["boxes"], att_masks=tb["att_masks"],
                                opt=dict(opts, beam_size=b, group_size=G), mode="sample")
        p_r = np.array([[d["p"] for d in db] for db in model.done_beams], np.float32)
        assert torch.equal(seq_r, seq), f"{name}: diverse_beam_ref and the repaired reference decode different tokens"
        assert int((gap >= D.GAP).sum()) >= need
        print(name, "seed", seed, "min_gap", gap.tolist(), "max |lp - ref|", float((lp_r - lp).abs().max()),
              "max |p - ref|", float(np.abs(p_r - p.numpy()).max()))
        g[f"{name}/seed"] = np.int64(seed)
        g[f"{name}/seq"] = seq_r.numpy()
        g[f"{name}/logprobs"] = lp_r.numpy()
        g[f"{name}/p"] = p_r
        g[f"{name}/min_gap"] = gap.numpy()
    C.save_golden(os.path.join(HERE, "g16_diverse_beam.npz"), g)


if __name__ == "__main__":
    main()
