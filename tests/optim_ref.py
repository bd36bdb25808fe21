"""Numpy fp32 restatement of the native optimiser family (include/ortk.h: ortk_optim_step) and of the three learning-rate
schedules of the reference's utils/optim.py: clip_grad_value_ followed by torch 2.x's single-tensor rules, one fp32 rounding per
operation, in the order the header states.  The schedules are plain Python floats (double), as the reference computes them.

Shared by tests/test_optim_host.py (against torch.optim on the CPU and against golden G17) and tests/test_gpu_optim.py (the
device operator against this restatement)."""
import math

import numpy as np

KINDS = ("adam", "sgd", "sgdm", "sgdmom", "rmsprop", "adagrad")
N_STATES = {"adam": 2, "sgd": 0, "sgdm": 1, "sgdmom": 1, "rmsprop": 1, "adagrad": 1}
F = np.float32

# Operator-test inputs (the issue's): n = 4099, p ~ N(0, 0.1^2), gradients alternating between scales 0.3 and 0.02, clip 0.1, 6 steps.
OP_N, OP_STEPS, OP_CLIP = 4099, 6, 0.1
# One hyper-parameter set per kind: (lr, alpha, beta, eps).  Rates keep |p| < 0.6 over the 6 steps and move p by more than 1e-2.
# alpha / beta are dyadic (0.875 = 1 - 2^-3, 0.984375 = 1 - 2^-6, 0.99609375 = 1 - 2^-8), so that `1 - beta` is the same number whether
# it is formed in fp32 (the kernels, as adam_clip_kernel always has: 1.f - b) or in double and then rounded (torch).  With decimal
# betas the two differ (1.f - 0.999f = 0.0010000467), which is a property of the constants, not of the update rule under test.
OP_HYPER = {
    "adam": (0.01, 0.875, 0.99609375, 1e-8),
    "sgd": (0.5, 0.0, 0.0, 0.0),
    "sgdm": (0.2, 0.875, 0.0, 0.0),
    "sgdmom": (0.2, 0.875, 0.0, 0.0),
    "rmsprop": (0.01, 0.984375, 0.0, 1e-8),
    "adagrad": (0.05, 0.0, 0.0, 1e-10),
}
# Largest |restatement - torch.optim| over all kinds and both weight decays at these inputs, measured by
# test_optim_host.py::test_restatement_vs_torch_optim: 8.94e-8 = 1.5 x 2^-24 (rmsprop, weight_decay 0; every other kind is at or below
# 5.96e-8, one ulp of a value in [0.5, 1)).  That test prints the figures; the device bar (tests/test_gpu_optim.py) is 4 x this.
HOST_DISTANCE = 1.5 * 2.0 ** -24


def op_inputs(n=OP_N, steps=OP_STEPS, seed=0):
    rs = np.random.RandomState(1234 + seed)
    p0 = (0.1 * rs.standard_normal(n)).astype(F)
    grads = [((0.3 if s % 2 == 0 else 0.02) * rs.standard_normal(n)).astype(F) for s in range(steps)]
    return p0, grads


def new_state(kind, n):
    return [np.zeros(n, F) for _ in range(N_STATES[kind])]


def step(kind, p, g, state, t, lr, alpha=0.9, beta=0.999, eps=1e-8, weight_decay=0.0, clip=0.1, first_step=None):
    """One update in place on fp32 arrays `p` and `state` (a list of N_STATES[kind] arrays); `t` = 1-based step count (Adam's bias
    corrections, and the momentum kinds' first step unless `first_step` says otherwise).  Returns p."""
    assert p.dtype == F and g.dtype == F and all(s.dtype == F for s in state)
    bc1, bc2 = 1.0 - float(alpha) ** t, 1.0 - float(beta) ** t          # double, as torch and the native host side compute them
    lr, alpha, beta, eps, wd, clip = F(lr), F(alpha), F(beta), F(eps), F(weight_decay), F(clip)
    one = F(1.0)
    gc = np.minimum(np.maximum(g, -clip), clip)
    if wd != 0:
        gc = gc + wd * p
    if kind == "adam":
        m, v = state
        step_size, sqrt_bc2 = F(lr / F(bc1)), F(math.sqrt(float(F(bc2))))
        m[:] = m + (gc - m) * (one - alpha)
        v[:] = v * beta + gc * gc * (one - beta)
        denom = np.sqrt(v) / sqrt_bc2 + eps
        p[:] = p - step_size * (m / denom)
    elif kind == "sgd":
        p[:] = p - lr * gc
    elif kind in ("sgdm", "sgdmom"):
        buf, = state
        first = (t == 1) if first_step is None else bool(first_step)
        buf[:] = gc if first else alpha * buf + gc
        p[:] = p - lr * (buf if kind == "sgdm" else gc + alpha * buf)
    elif kind == "rmsprop":
        sq, = state
        sq[:] = alpha * sq + (one - alpha) * gc * gc
        p[:] = p - lr * (gc / (np.sqrt(sq) + eps))
    elif kind == "adagrad":
        acc, = state
        acc[:] = acc + gc * gc
        p[:] = p - lr * (gc / (np.sqrt(acc) + eps))
    else:
        raise ValueError(kind)
    return p


# ---------------------------------------------------------------------------------------------- schedules (utils/optim.py)
def noam_rate(step, d_model, factor, warmup):
    return factor * (d_model ** (-0.5) * min(step ** (-0.5), step * warmup ** (-1.5)))


def step_rate(epoch, lr, decay_start, decay_every, decay_rate):
    if epoch > decay_start >= 0:
        return lr * decay_rate ** ((epoch - decay_start) // decay_every)
    return lr


def cosine_rate(step, max_train_step, lr, lr_min):
    s = 1.0 + math.cos(min(1.0, step / max_train_step) * math.pi)
    return (lr - lr_min) * (s / 2) + lr_min


def rate(scheduler, step, epoch, cfg):
    """`step`: the already incremented step count (RateOpt.step increments before rate()); cfg: dict of the reference's names."""
    if scheduler == "noam":
        return noam_rate(step, cfg["d_model"], cfg["noamopt_factor"], cfg["noamopt_warmup"])
    if scheduler == "step":
        return step_rate(epoch, cfg["learning_rate"], cfg["learning_rate_decay_start"], cfg["learning_rate_decay_every"],
                         cfg["learning_rate_decay_rate"])
    if scheduler == "cosine":
        return cosine_rate(step, cfg["max_train_step"], cfg["learning_rate"], cfg["learning_rate_min"])
    raise ValueError(scheduler)


# ---------------------------------------------------------------------------------------------- golden G17
# The cases of tests/golden/make_golden_optim.py: name -> the reference's config names that differ from its defaults
# (utils/training.py:409-473).  The generator, the host restatement and the native trainer all read this table.
G17_DEFAULTS = dict(optim="adam", lr_scheduler="noam", learning_rate=1e-2, learning_rate_min=1e-5, learning_rate_decay_start=0,
                    learning_rate_decay_every=3, learning_rate_decay_rate=0.8, optim_alpha=0.9, optim_beta=0.999, optim_epsilon=1e-8,
                    weight_decay=0.0, max_train_step=100, noamopt_factor=1.0, noamopt_warmup=10)
G17_STEPS, G17_CLIP = 3, 0.1
G17_DENSE = {
    "step_adam": dict(lr_scheduler="step", optim="adam", learning_rate=0.02, learning_rate_decay_start=0, learning_rate_decay_every=1,
                      learning_rate_decay_rate=0.5),
    "cosine_adam": dict(lr_scheduler="cosine", optim="adam", learning_rate=0.03, weight_decay=1e-2, optim_epsilon=1e-2, max_train_step=4),
    "step_sgd": dict(lr_scheduler="step", optim="sgd", learning_rate=1.0),
    "step_sgdm": dict(lr_scheduler="step", optim="sgdm", learning_rate=0.5),
    "step_sgdmom": dict(lr_scheduler="step", optim="sgdmom", learning_rate=0.3, weight_decay=1e-3),
    "cosine_rmsprop": dict(lr_scheduler="cosine", optim="rmsprop", learning_rate=0.02, optim_epsilon=1e-2, max_train_step=4),
    "step_adagrad": dict(lr_scheduler="step", optim="adagrad", learning_rate=0.05),
    "noam_sgd": dict(lr_scheduler="noam", optim="sgd"),
}
# masked cases: tiny relation_transformer_prune, supermask, as golden G13 (make_golden_maskopt.py) builds it
G17_MASKED = {
    "masked_step_adam": dict(lr_scheduler="step", optim="adam", learning_rate=0.02, optim_beta=0.98, optim_epsilon=1e-9),
    "masked_cosine_rmsprop": dict(lr_scheduler="cosine", optim="rmsprop", learning_rate=0.02, optim_epsilon=1e-2, max_train_step=4),
}
G17_MASK = dict(lr_mask={"masked_step_adam": 100.0, "masked_cosine_rmsprop": 1.0}, target=0.9, weight=30.0)      # (the sparsity loss ramps over the case's max_train_step)
G17_PARAMS = ("model.encoder.layers.0.self_attn.WGs.3.weight", "model.decoder.layers.1.src_attn.linears.2.bias",
              "model.decoder.norm.a_2", "model.generator.proj.bias")
G17_MASK_PARAM = "model.decoder.layers.1.feed_forward.w_1.weight_pruning_mask"


def g17_config(case):
    over = G17_DENSE.get(case) or G17_MASKED[case]
    return dict(G17_DEFAULTS, **over)


def optim_hyper(cfg):
    """(alpha, beta, eps) the chosen optimiser runs with under config `cfg` (utils/optim.py:149-174; adagrad keeps torch's 1e-10)."""
    kind = cfg["optim"]
    eps = 1e-10 if kind == "adagrad" else cfg["optim_epsilon"]
    return cfg["optim_alpha"], cfg["optim_beta"], eps
