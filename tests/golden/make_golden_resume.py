#!/usr/bin/env python3
"""Golden G18: the reference's resume flow (``--resume_training``) on the tiny models.

Every case runs steps 0 and 1 of zero_grad / forward / XE / backward / clip_gradient(0.1) / opt.step(epoch=step) with the optimiser
``optim.get_optim`` builds from the case's config (tests/resume_ref.py), takes ``copy.deepcopy(opt.state_dict())`` — through
``RateOpt.__getattr__`` that is the INNER torch.optim state — builds a new ``get_optim`` optimiser over the same model, loads the
dict into it as ``maybe_load_checkpoint`` does (utils/training.py:181-185) and runs steps 2 and 3.  The new wrapper counts from 0
again and so does the loop's ``global_step`` (utils/training.py:136): the rate and the sparsity-loss ramp restart, the moments and
Adam's ``step`` continue.  Models, batch, clip and injected Bernoulli draws are those of golden G17 (make_golden_optim.py).

Per case: four losses, four rates (float64), the G17 parameters (plus one mask tensor for the masked case), param_abs_sum and the
parameter names of every param group in the order the reference's optimiser holds them.

Power, asserted: every stored tensor of the resumed run lies at least 1e-2 — 20 x the 5e-4 comparison bar — from the same run with
a second optimiser that was NOT loaded and, for the schedules that depend on the step count (noam, cosine), from the uninterrupted
four-step run.  Run in the build container only:
    python tests/golden/make_golden_resume.py
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import common as C  # noqa: E402
import resume_ref as RR  # noqa: E402
from make_golden import import_reference, load_weights, tt  # noqa: E402
from make_golden_maskopt import draws_for  # noqa: E402
from make_golden_optim import checksum  # noqa: E402


def main():
    get_model, Config, losses, optim, prune = import_reference()
    import torch
    torch.manual_seed(0)
    torch.set_num_threads(4)
    tb = tt(C.make_inputs(**C.G1_INPUTS))
    crit = losses.LanguageModelCriterion()
    M = RR.G18_MASK
    out = {}

    def build(case):
        cfgd = RR.g18_config(case)
        masked = case in RR.G18_MASKED
        if masked:
            cfg = Config(**dict(C.TINY_CFG, prune_type="supermask", prune_mask_freeze_scope="model.generator.", prune_supermask_init=5.0))
            model = get_model("relation_transformer_prune")(cfg)
            load_weights(model, C.G1_SEED, C.G1_GEN_SCALE, C.G1_EOS_BIAS, keep_prob=C.G3_KEEP)
            model.train()
            for m_ in model.modules():
                if isinstance(m_, torch.nn.Dropout):
                    m_.p = 0.0
        else:
            cfg = Config(**C.TINY_CFG)
            model = get_model("relation_transformer")(cfg)
            load_weights(model, C.G1_SEED, C.G1_GEN_SCALE, C.G1_EOS_BIAS)
            model.eval()                                   # dropout off, parameters train

        def new_opt():
            if masked:                                     # scripts/train_n_prune_transformer.py:67-82
                params = [{"params": list(model.all_weights(named=False))},
                          {"params": list(model.active_pruning_masks(named=False)), "lr": M["lr_mask"], "weight_decay": 0, "eps": 1e-2,
                           "pruning_mask": True}]
            else:
                params = model.parameters()
            return optim.get_optim(params, Config(d_model=cfg.d_model, **cfgd))
        return model, new_opt, cfgd, masked

    def steps(model, opt, masked, cfgd, which, global_step, losses_out, rates_out):
        """Steps `which` (their number is the `epoch` and keys the injected draws); `global_step` counts as the loop's does."""
        orig = torch.bernoulli
        try:
            for step in which:
                if masked:
                    torch.bernoulli = lambda p, *a, _s=step, **k: (torch.from_numpy(draws_for(p.shape, _s)) < p).to(p.dtype)
                opt.zero_grad()
                logp = model(att_feats=tb["att_feats"], boxes=tb["boxes"], seqs=tb["seqs"], att_masks=tb["att_masks"])
                loss = crit(logp, tb["seqs"][:, 1:], tb["masks"][:, 1:])
                if masked:
                    loss = loss + model.compute_sparsity_loss(M["target"], weight=M["weight"], current_step=global_step,
                                                              max_step=cfgd["max_train_step"])
                loss.backward()
                optim.clip_gradient(opt, RR.G18_CLIP)
                opt.step(epoch=step)
                global_step += 1
                losses_out.append(loss.item())
                rates_out.append(opt.rate())
        finally:
            torch.bernoulli = orig

    def run(case, how):
        """how: "resume" (second optimiser loaded), "fresh" (second optimiser not loaded) or "straight" (one optimiser, four steps)."""
        model, new_opt, cfgd, masked = build(case)
        opt = new_opt()
        ls, rs = [], []
        first, second = range(RR.G18_SPLIT), range(RR.G18_SPLIT, RR.G18_STEPS)
        steps(model, opt, masked, cfgd, first, 0, ls, rs)
        if how == "straight":
            steps(model, opt, masked, cfgd, second, RR.G18_SPLIT, ls, rs)
            return model, opt, ls, rs
        saved = copy.deepcopy(opt.state_dict())
        opt2 = new_opt()
        if how == "resume":
            opt2.load_state_dict(saved)
        steps(model, opt2, masked, cfgd, second, 0, ls, rs)
        return model, opt2, ls, rs

    for case in list(RR.G18_DENSE) + list(RR.G18_MASKED):
        masked = case in RR.G18_MASKED
        names = RR.G18_PARAMS + ((RR.G18_MASK_PARAM,) if masked else ())
        model, opt, ls, rs = run(case, "resume")
        sd = {n: p.detach().numpy().copy() for n, p in model.named_parameters()}
        out[f"{case}/losses"] = np.array(ls, np.float32)
        out[f"{case}/rates"] = np.array(rs, np.float64)
        for n in names:
            out[f"{case}/param/{n}"] = sd[n]
        out[f"{case}/param_abs_sum"] = checksum(model.named_parameters())
        by_id = {id(p): n for n, p in model.named_parameters()}
        for gi, group in enumerate(opt.optimizer.param_groups):
            out[f"{case}/group{gi}_names"] = np.array([by_id[id(p)] for p in group["params"]])
        out[f"{case}/n_groups"] = np.int64(len(opt.optimizer.param_groups))
        if masked:
            out[f"{case}/mask_abs_sum"] = np.float64(sum(p.detach().double().abs().sum().item() for _, p in model.all_pruning_masks()))
            assert opt.optimizer.param_groups[1]["lr"] == M["lr_mask"] and opt.optimizer.param_groups[1]["pruning_mask"] is True
        # power: a resume that loaded nothing, or one that kept the schedule running, is told apart from the reference's
        others = ["fresh"] + (["straight"] if RR.g18_config(case)["lr_scheduler"] in RR.STEP_SCHEDULES else [])
        for how in others:
            other = dict(run(case, how)[0].named_parameters())
            diffs = {n: float(np.abs(other[n].detach().numpy() - sd[n]).max()) for n in names}
            print(case, "vs", how, {n.split(".")[-2] + "." + n.split(".")[-1]: round(d, 4) for n, d in diffs.items()})
            for n, d in diffs.items():
                assert d >= RR.MIN_DIFF, (case, how, n, d)
        print(case, "losses", ls, "rates", rs)

    path = os.path.join(HERE, "g18_tiny_resume.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
