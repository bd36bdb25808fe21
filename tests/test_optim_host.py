"""Host-side checks of the optimiser family (no GPU): the numpy fp32 restatement (tests/optim_ref.py) against torch.optim on the CPU
and against golden G17 (the reference's own runs, tests/golden/make_golden_optim.py), the three learning-rate schedules at
hand-checked points, and the trainer's option parsing."""
import warnings
import zlib

import numpy as np
import pytest
import torch

import common as C
import helpers as H
import optim_ref as R
from oracle import ort_oracle as O

F = np.float32


def _torch_optimizer(kind, p, lr, alpha, beta, eps, wd):
    kw = dict(foreach=False)
    if kind == "adam":
        return torch.optim.Adam([p], lr, (alpha, beta), eps, weight_decay=wd, **kw)
    if kind == "sgd":
        return torch.optim.SGD([p], lr, weight_decay=wd, **kw)
    if kind == "sgdm":
        return torch.optim.SGD([p], lr, alpha, weight_decay=wd, **kw)
    if kind == "sgdmom":
        return torch.optim.SGD([p], lr, alpha, weight_decay=wd, nesterov=True, **kw)
    if kind == "rmsprop":
        return torch.optim.RMSprop([p], lr, alpha, eps, weight_decay=wd, **kw)
    return torch.optim.Adagrad([p], lr, weight_decay=wd, **kw)


def test_restatement_vs_torch_optim(capsys):
    """6 steps, all six kinds, weight_decay 0 and 1e-2.  torch contracts some multiplies and adds, so the result is never bit-equal;
    the bar is one fp32 ulp at 1.0."""
    p0, grads = R.op_inputs()
    worst = {}
    for kind in R.KINDS:
        lr, alpha, beta, eps = R.OP_HYPER[kind]
        for wd in (0.0, 1e-2):
            p, state = p0.copy(), R.new_state(kind, p0.size)
            tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
            opt = _torch_optimizer(kind, tp, lr, alpha, beta, eps, wd)
            for t, g in enumerate(grads, 1):
                R.step(kind, p, g, state, t, lr, alpha, beta, eps, wd, R.OP_CLIP)
                tp.grad = torch.from_numpy(g.copy())
                torch.nn.utils.clip_grad_value_([tp], R.OP_CLIP)
                opt.step()
            assert float(np.abs(p).max()) < 0.6 and float(np.abs(p - p0).max()) > 1e-2, (kind, wd)     # moved, and stayed in range
            worst[(kind, wd)] = float(np.abs(p - tp.detach().numpy()).max())
    with capsys.disabled():
        print("\nrestatement vs torch.optim, max |diff|:", {f"{k}/wd={w:g}": f"{v:.2e}" for (k, w), v in worst.items()})
    assert max(worst.values()) <= 1.2e-7, worst
    # (optim_ref.HOST_DISTANCE, from which the device bar is derived, records the largest figure printed above: 8.94e-8; torch's CPU
    #  kernels may contract differently on another host, so only the one-ulp bar is asserted)


# ---------------------------------------------------------------------------------------------- golden G17
def _draws(shape, step):
    rs = np.random.RandomState((zlib.crc32(str(tuple(shape)).encode()) + 7919 * step) & 0x7FFFFFFF)
    return rs.uniform(size=tuple(shape)).astype(F)


def _apply(cfg, names, P, states, t, lr, eps, wd):
    alpha, beta, _ = R.optim_hyper(cfg)
    for n in names:
        g = P[n].grad
        g = np.zeros(tuple(P[n].shape), F) if g is None else g.numpy().reshape(-1)
        R.step(cfg["optim_kind"], P[n].detach().numpy().reshape(-1), np.ascontiguousarray(g, F), states[n], t, lr, alpha, beta, eps, wd,
               R.G17_CLIP)


def _restate(case, masked):
    cfg = R.g17_config(case)
    noam = cfg["lr_scheduler"] == "noam"
    cfg["optim_kind"] = "adam" if noam else cfg["optim"]
    if noam:                                           # get_optim: Adam(betas 0.9 / 0.98, eps 1e-9), no weight decay
        cfg.update(optim="adam", optim_alpha=0.9, optim_beta=0.98, optim_epsilon=1e-9, weight_decay=0.0)
    cfg["d_model"] = C.TINY_CFG["d_model"]
    ocfg = O.OCfg(**{k: v for k, v in C.TINY_CFG.items() if not k.startswith("prune")})
    b = H.g1_batch()
    if masked:
        P = H.torch_state(H.prune_param_shapes(C.TINY_CFG), C.G1_SEED, C.G1_GEN_SCALE, C.G1_EOS_BIAS, keep_prob=C.G3_KEEP,
                          requires_grad=True)
    else:
        P = H.g1_state(requires_grad=True)
    weights = [n for n in P if not O.is_mask(n)]
    active = [n for n in P if O.is_mask(n) and not n.startswith("model.generator.")]          # prune_mask_freeze_scope
    kind = cfg["optim_kind"]
    states = {n: R.new_state(kind, P[n].numel()) for n in P}
    _, _, eps = R.optim_hyper(cfg)
    M = R.G17_MASK
    losses, rates = [], []
    for step in range(R.G17_STEPS):
        for p in P.values():
            p.grad = None
        if masked:
            samples = {n: (torch.from_numpy(_draws(P[n].shape, step)) < torch.sigmoid(P[n].detach())).float() for n in P if O.is_mask(n)}
            E = O.effective_params(P, "supermask", training=True, samples=samples)
        else:
            E = P
        logp = O.forward_logp(E, ocfg, b["att_feats"], b["boxes"], b["seqs"], b["att_masks"])
        loss = O.xe_loss(logp, b["seqs"][:, 1:], b["masks"][:, 1:])
        if masked:
            # (compute_sparsity_loss counts the ACTIVE masks only, prune.py:240; it ramps over the run's max_train_step)
            loss = loss + O.sparsity_loss({n: P[n] for n in active}, M["target"], M["weight"], step, cfg["max_train_step"])
        loss.backward()
        losses.append(loss.item())
        lr = R.rate(cfg["lr_scheduler"], step + 1, step, cfg)
        rates.append(lr)
        with torch.no_grad():
            _apply(cfg, weights, P, states, step + 1, lr, eps, cfg["weight_decay"])
            if masked:                                 # second param group: same kind, its own lr, eps 1e-2, no weight decay, no scheduler
                _apply(cfg, active, P, states, step + 1, M["lr_mask"][case], 1e-2, 0.0)
    return P, losses, rates


@pytest.mark.parametrize("case", list(R.G17_DENSE) + list(R.G17_MASKED))
def test_restatement_vs_reference_golden(golden, case):
    """The restatement on the oracle's gradients against the reference's runs, at G4's bars (test_oracle_golden.py)."""
    g17 = golden("g17_tiny_optim_family")
    masked = case in R.G17_MASKED
    P, losses, rates = _restate(case, masked)
    np.testing.assert_allclose(rates, g17[f"{case}/rates"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(losses, g17[f"{case}/losses"], rtol=0, atol=5e-4)
    n_checked = 0
    for k, v in g17.items():
        if k.startswith(f"{case}/param/"):
            name = k[len(case) + 7:]
            if O.is_mask(name):
                # a logit moves by lr_mask * O(1) per step on 1e-7 gradient noise: G13's bar (test_gpu_model.py)
                np.testing.assert_allclose(P[name].detach().numpy(), v, rtol=2e-3, atol=5e-2, err_msg=k)
            else:
                np.testing.assert_allclose(P[name].detach().numpy(), v, rtol=0, atol=5e-4, err_msg=k)
            n_checked += 1
    assert n_checked == (5 if masked else 4)
    tot = sum(p.detach().double().abs().sum().item() for n, p in P.items() if not n.endswith("attn.linears.1.bias"))
    assert abs(tot - float(g17[f"{case}/param_abs_sum"])) / tot < 1e-4


def test_golden_noam_ignores_optim(golden):
    g17, g4 = golden("g17_tiny_optim_family"), golden("g4_tiny_optim")
    np.testing.assert_array_equal(g17["noam_sgd/losses"], g4["losses"])
    np.testing.assert_array_equal(g17["noam_sgd/rates"], g4["rates"])
    np.testing.assert_array_equal(g17["noam_sgd/param/model.generator.proj.bias"], g4["param/model.generator.proj.bias"])
    assert float(g17["noam_sgd/param_abs_sum"]) == float(g4["param_abs_sum"])


# ---------------------------------------------------------------------------------------------- schedules
def test_schedules_at_hand_checked_points():
    from sparse_image_captioning_amd.training import OptimSpec
    # noam: factor * d^-0.5 * min(step^-0.5, step * warmup^-1.5)
    s = OptimSpec(512, noamopt_factor=2.0, noamopt_warmup=4)
    assert s.rate(1) == pytest.approx(2.0 * 512 ** -0.5 * 1 / 8) and s.rate(4) == pytest.approx(2.0 * 512 ** -0.5 * 0.5)
    assert s.rate(16) == pytest.approx(2.0 * 512 ** -0.5 * 0.25) and s.rate(0) == s.rate(1)
    # step: decays only when epoch > decay_start >= 0
    s = OptimSpec(512, lr_scheduler="step", learning_rate=0.1, learning_rate_decay_start=2, learning_rate_decay_every=3, learning_rate_decay_rate=0.5)
    assert [s.rate(9, e) for e in (0, 2, 3, 4, 5, 7, 8)] == [0.1, 0.1, 0.1, 0.1, 0.05, 0.05, 0.025]
    s = OptimSpec(512, lr_scheduler="step", learning_rate=5e-5, learning_rate_decay_start=-1)          # the SCST recipes: constant
    assert [s.rate(1, e) for e in (0, 1, 50)] == [5e-5] * 3
    s = OptimSpec(512, lr_scheduler="step", learning_rate=0.1, learning_rate_decay_start=0, learning_rate_decay_every=1, learning_rate_decay_rate=0.5)
    assert [s.rate(1, e) for e in (0, 1, 2)] == [0.1, 0.05, 0.025]
    # cosine: the already incremented step over max_train_step, clamped at 1
    s = OptimSpec(512, lr_scheduler="cosine", learning_rate=0.01, learning_rate_min=0.002, max_train_step=4)
    assert s.rate(2) == pytest.approx(0.006) and s.rate(4) == pytest.approx(0.002) and s.rate(9) == pytest.approx(0.002)
    assert s.rate(1) == pytest.approx(0.008 * (1 + 2 ** -0.5) / 2 + 0.002) and s.rate(0) == pytest.approx(0.01)
    # the restatement's schedules are the same functions
    cfg = dict(R.G17_DEFAULTS, d_model=512, learning_rate=0.01, learning_rate_min=0.002, max_train_step=4)
    assert R.rate("cosine", 1, 0, cfg) == s.rate(1) and R.rate("noam", 3, 0, cfg) == OptimSpec(512, noamopt_warmup=10).rate(3)


# ---------------------------------------------------------------------------------------------- options
def test_option_parsing():
    import sparse_image_captioning_amd.training as T
    from sparse_image_captioning_amd.utils.config import Config
    cfg = Config(optim="RMSprop", lr_scheduler="cosine", learning_rate=0.01, learning_rate_min=1e-4, optim_alpha=0.95, optim_epsilon=0.01,
                 weight_decay=1e-3, max_train_step=1000, d_model=512, some_other_name=3)
    opts = T.OptimSpec.options_from_config(cfg)
    assert opts == dict(optim="RMSprop", lr_scheduler="cosine", learning_rate=0.01, learning_rate_min=1e-4, optim_alpha=0.95,
                        optim_epsilon=0.01, weight_decay=1e-3, max_train_step=1000)
    s = T.OptimSpec(512, **opts)
    assert (s.kind, s.alpha, s.eps, s.weight_decay, s.n_states, s.plain_adam) == ("rmsprop", 0.95, 0.01, 1e-3, 1, False)
    assert s.rate(500) == pytest.approx((0.01 - 1e-4) / 2 + 1e-4)
    # the reference's defaults (utils/training.py:409-473)
    d = T.OptimSpec(512, lr_scheduler="step")
    assert (d.kind, d.alpha, d.beta, d.eps, d.weight_decay, d.learning_rate, d.decay_every, d.decay_rate) == ("adam", 0.9, 0.999, 1e-8, 0.0, 5e-4, 3, 0.8)
    assert T.OptimSpec(512, lr_scheduler="step", optim="adagrad", optim_epsilon=0.5).eps == 1e-10
    assert [T.OptimSpec(512, lr_scheduler="step", optim=k).n_states for k in ("adam", "sgd", "sgdm", "sgdmom", "rmsprop", "adagrad")] == [2, 0, 1, 1, 1, 1]
    # noam ignores optim and weight_decay, warns once, keeps Adam with the constructor's betas / eps
    T._noam_warned = False
    with pytest.warns(UserWarning, match="Ignoring optim choice"):
        n = T.OptimSpec(512, optim="sgd", weight_decay=0.1, optim_alpha=0.5)
    assert (n.kind, n.alpha, n.beta, n.eps, n.weight_decay, n.plain_adam) == ("adam", 0.9, 0.98, 1e-9, 0.0, True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        T.OptimSpec(512, optim="rmsprop")
    # unknown names are refused, before any device work (the model argument is never touched beyond d_model)
    for bad in (dict(optim="adamw"), dict(lr_scheduler="linear"), dict(learning_rates=0.1)):
        with pytest.raises(ValueError):
            T.OptimSpec(512, **bad)
    for bad in (dict(lr_scheduler="step", learning_rate_decay_rate=1.5), dict(lr_scheduler="step", learning_rate_decay_every=0),
                dict(lr_scheduler="cosine", max_train_step=0), dict(lr_scheduler="step", learning_rate=float("nan"))):
        with pytest.raises(ValueError):
            T.OptimSpec(512, **bad)

    class FakeModel:
        d_model = 512
    with pytest.raises(ValueError):
        T.NativeTrainer(FakeModel(), optim="adamw", lr_scheduler="step")
    with pytest.raises(ValueError):
        T.NativeTrainer.from_config(FakeModel(), Config(lr_scheduler="exponential"))
    with pytest.raises(TypeError):
        T.NativeTrainer.from_config(FakeModel(), Config(), no_such_argument=1)
