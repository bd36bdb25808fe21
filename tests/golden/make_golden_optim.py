#!/usr/bin/env python3
"""Golden G17: the reference's optimiser family and learning-rate schedules on the tiny models.

Every case runs 3 steps of zero_grad / forward / XE / backward / clip_gradient(0.1) / opt.step(epoch=step) with the optimiser that
the reference's ``optim.get_optim`` builds from the case's config (tests/optim_ref.py: G17_DENSE, G17_MASKED).

  dense cases   the G1 tiny model and batch under model.eval() (dropout off), as golden G4
  masked cases  the tiny relation_transformer_prune (supermask) with the reference's two param groups, injected Bernoulli draws,
                sparsity loss and frozen generator masks, as golden G13 (make_golden_maskopt.py)

Per case: losses, rates (float64), four small parameters (a WG weight, a bias, a LayerNorm gain, generator.proj.bias), for the masked
cases one mask tensor, and param_abs_sum as in G4 (key-projection biases excluded).  The learning rates are chosen so that every
stored tensor moves by at least 1e-2 — 20 x the 5e-4 comparison bar — and that is asserted: a trainer that never updated fails.
Run in the build container only:
    python tests/golden/make_golden_optim.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import common as C  # noqa: E402
import optim_ref as R  # noqa: E402
from make_golden import import_reference, load_weights, tt  # noqa: E402
from make_golden_maskopt import draws_for  # noqa: E402

MIN_MOVE = 1e-2


def checksum(named):
    return np.float64(sum(p.detach().double().abs().sum().item() for n, p in named if not n.endswith("attn.linears.1.bias")))


def main():
    get_model, Config, losses, optim, prune = import_reference()
    import torch
    torch.manual_seed(0)
    torch.set_num_threads(4)
    tb = tt(C.make_inputs(**C.G1_INPUTS))
    crit = losses.LanguageModelCriterion()
    out = {}

    def record(case, model, before, step_losses, rates, names):
        sd = dict(model.named_parameters())
        out[f"{case}/losses"] = np.array(step_losses, np.float32)
        out[f"{case}/rates"] = np.array(rates, np.float64)
        for n in names:
            v = sd[n].detach().numpy().copy()
            move = float(np.abs(v - before[n]).max())
            assert move >= MIN_MOVE, (case, n, move)
            out[f"{case}/param/{n}"] = v
        out[f"{case}/param_abs_sum"] = checksum(model.named_parameters())
        print(case, "losses", step_losses, "rates", rates, "moves",
              [round(float(np.abs(sd[n].detach().numpy() - before[n]).max()), 4) for n in names])

    # ------------------------------------------------------------------ dense
    for case in R.G17_DENSE:
        cfgd = R.g17_config(case)
        cfg = Config(**C.TINY_CFG)
        model = get_model("relation_transformer")(cfg)
        load_weights(model, C.G1_SEED, C.G1_GEN_SCALE, C.G1_EOS_BIAS)
        model.eval()                                   # dropout off, parameters train
        before = {n: p.detach().numpy().copy() for n, p in model.named_parameters()}
        opt = optim.get_optim(model.parameters(), Config(d_model=cfg.d_model, **cfgd))
        step_losses, rates = [], []
        for step in range(R.G17_STEPS):
            opt.zero_grad()
            logp = model(att_feats=tb["att_feats"], boxes=tb["boxes"], seqs=tb["seqs"], att_masks=tb["att_masks"])
            loss = crit(logp, tb["seqs"][:, 1:], tb["masks"][:, 1:])
            loss.backward()
            optim.clip_gradient(opt, R.G17_CLIP)
            opt.step(epoch=step)
            step_losses.append(loss.item())
            rates.append(opt.rate())
        record(case, model, before, step_losses, rates, R.G17_PARAMS)
    # noam ignores `optim`: the run is G4's Adam run
    g4 = np.load(os.path.join(HERE, "g4_tiny_optim.npz"))
    np.testing.assert_array_equal(out["noam_sgd/losses"], g4["losses"])
    np.testing.assert_array_equal(out["noam_sgd/rates"], g4["rates"])
    for n in ("model.encoder.layers.0.self_attn.WGs.3.weight", "model.generator.proj.bias"):
        np.testing.assert_array_equal(out["noam_sgd/param/" + n], g4["param/" + n])
    assert float(out["noam_sgd/param_abs_sum"]) == float(g4["param_abs_sum"])

    # ------------------------------------------------------------------ masked (supermask, two param groups)
    M = R.G17_MASK
    for case in R.G17_MASKED:
        cfgd = R.g17_config(case)
        cfg = Config(**dict(C.TINY_CFG, prune_type="supermask", prune_mask_freeze_scope="model.generator.", prune_supermask_init=5.0))
        model = get_model("relation_transformer_prune")(cfg)
        load_weights(model, C.G1_SEED, C.G1_GEN_SCALE, C.G1_EOS_BIAS, keep_prob=C.G3_KEEP)
        model.train()
        for m_ in model.modules():
            if isinstance(m_, torch.nn.Dropout):
                m_.p = 0.0
        before = {n: p.detach().numpy().copy() for n, p in model.named_parameters()}
        groups = [{"params": list(model.all_weights(named=False))},
                  {"params": list(model.active_pruning_masks(named=False)), "lr": M["lr_mask"][case], "weight_decay": 0, "eps": 1e-2,
                   "pruning_mask": True}]
        opt = optim.get_optim(groups, Config(d_model=cfg.d_model, **cfgd))
        step_losses, rates = [], []
        orig = torch.bernoulli
        try:
            for step in range(R.G17_STEPS):
                torch.bernoulli = lambda p, *a, _s=step, **k: (torch.from_numpy(draws_for(p.shape, _s)) < p).to(p.dtype)
                opt.zero_grad()
                logp = model(att_feats=tb["att_feats"], boxes=tb["boxes"], seqs=tb["seqs"], att_masks=tb["att_masks"])
                loss = crit(logp, tb["seqs"][:, 1:], tb["masks"][:, 1:])
                loss = loss + model.compute_sparsity_loss(M["target"], weight=M["weight"], current_step=step,
                                                          max_step=cfgd["max_train_step"])
                loss.backward()
                optim.clip_gradient(opt, R.G17_CLIP)
                opt.step(epoch=step)
                step_losses.append(loss.item())
                rates.append(opt.rate())
        finally:
            torch.bernoulli = orig
        assert opt.optimizer.param_groups[1]["lr"] == M["lr_mask"][case]          # no scheduler touches the mask group
        record(case, model, before, step_losses, rates, R.G17_PARAMS + (R.G17_MASK_PARAM,))
        out[f"{case}/mask_abs_sum"] = np.float64(sum(p.detach().double().abs().sum().item() for _, p in model.all_pruning_masks()))
        gm = dict(model.named_parameters())["model.generator.proj.weight_pruning_mask"].detach().numpy()
        assert np.array_equal(gm, before["model.generator.proj.weight_pruning_mask"])      # frozen scope

    path = os.path.join(HERE, "g17_tiny_optim_family.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
