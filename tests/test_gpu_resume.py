"""Save and resume of ``NativeTrainer`` on the device: the reference's resume flow against golden G18 (the reference's own runs,
tests/golden/make_golden_resume.py), exact continuation through ``save_checkpoint`` / ``load_checkpoint`` — byte for byte on replayed
gradients, within the atomics' noise on real steps with dropout, token for token in an SCST step — and the state round trip."""
import os

import numpy as np
import pytest
import torch

import common as C
import helpers as H
import optim_ref as R
import resume_ref as RR

pytestmark = pytest.mark.gpu

MASKED_CFG = dict(prune_type="supermask", prune_mask_freeze_scope="model.generator.", prune_supermask_init=5.0)
SHARE_CFG = dict(C.TINY_CFG, num_layers=3, share_layer_encoder=(0, 1, 0), share_layer_decoder=(0, 0, 1))          # golden G8's


@pytest.fixture(scope="module")
def P():
    import sparse_image_captioning_amd as pkg
    pkg._lib.require_gpu()
    return pkg


def _model(P, name, cfg, state, **over):
    from sparse_image_captioning_amd.utils.config import Config
    m = P.get_model(name)(Config(**dict(cfg, **over)))
    missing, unexpected = m.load_state_dict(state, strict=False)
    assert not unexpected and all(k.endswith(".pe") or k.endswith("_pruning_mask") for k in missing), (missing, unexpected)
    return m.cuda().eval()


def _dense(P):
    return _model(P, "relation_transformer", C.TINY_CFG, H.g1_state())


def _masked(P, dropout=False):
    shapes = H.prune_param_shapes(C.TINY_CFG)
    state = H.torch_state(shapes, C.G1_SEED, C.G1_GEN_SCALE, C.G1_EOS_BIAS, keep_prob=C.G3_KEEP)
    m = _model(P, "relation_transformer_prune", C.TINY_CFG, state, **MASKED_CFG)
    m.train()
    if not dropout:
        m._ccfg.drop, m._ccfg.drop_src = 0.0, 0.0
    return m


def _trainer(m, cfg, mask_lr=RR.G18_MASK["lr_mask"], **kw):
    from sparse_image_captioning_amd.training import NativeTrainer
    if getattr(m, "MASKED", False):
        kw = dict(dict(prune_supermask_lr=mask_lr, mask_eps=1e-2, sparsity_target=RR.G18_MASK["target"],
                       sparsity_weight=RR.G18_MASK["weight"]), **kw)
    return NativeTrainer(m, grad_clip=RR.G18_CLIP, **dict(cfg, **kw))


def _batch():
    return {k: v.cuda() for k, v in H.g1_batch().items()}


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------- 1. the reference's resume, golden G18
def _check_case(g, case, m, losses, rates):
    """The bars of test_gpu_optim.py::_check_case, restated: rates 1e-12, losses 5e-4, parameters 5e-4 (a mask logit: rtol 2e-3, atol
    5e-2, golden G13's), checksum 1e-4 relative; the masked case's mask sum 2e-3 relative."""
    np.testing.assert_allclose(rates, g[f"{case}/rates"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(losses, g[f"{case}/losses"], rtol=0, atol=5e-4)
    sd = {n: p.detach().cpu().numpy() for n, p in m.named_parameters()}
    n_checked = 0
    for k, v in g.items():
        if k.startswith(f"{case}/param/"):
            name = k[len(case) + 7:]
            if name.endswith("_pruning_mask"):
                np.testing.assert_allclose(sd[name], v, rtol=2e-3, atol=5e-2, err_msg=k)
            else:
                np.testing.assert_allclose(sd[name], v, rtol=0, atol=5e-4, err_msg=k)
            n_checked += 1
    assert n_checked >= 4
    tot = sum(float(np.abs(v.astype(np.float64)).sum()) for n, v in sd.items() if not n.endswith("attn.linears.1.bias"))
    assert abs(tot - float(g[f"{case}/param_abs_sum"])) / tot < 1e-4
    if f"{case}/mask_abs_sum" in g:
        want = float(g[f"{case}/mask_abs_sum"])
        tot = sum(p.detach().double().abs().sum().item() for _, p in m.all_pruning_masks())
        assert abs(tot - want) / want < 2e-3


def _draws(shape, step):
    import zlib
    return np.random.RandomState((zlib.crc32(str(tuple(shape)).encode()) + 7919 * step) & 0x7FFFFFFF).uniform(size=tuple(shape)).astype(np.float32)


def _golden_steps(m, tr, b, steps, losses, rates):
    masked = getattr(m, "MASKED", False)
    mask_shapes = {k: v for k, v in H.prune_param_shapes(C.TINY_CFG).items() if k.endswith("_pruning_mask")} if masked else {}
    for step in steps:
        tr.epoch = step
        if masked:
            m.set_mask_draws({k: _draws(shp, step) for k, shp in mask_shapes.items()})
        losses.append(tr.xe_step(b, train=masked).item())
        rates.append(tr.rate())


@pytest.mark.parametrize("via", ["files", "memory"])
@pytest.mark.parametrize("case", list(RR.G18_DENSE) + list(RR.G18_MASKED))
def test_reference_resume_vs_reference_golden(P, golden, tmp_path, case, via):
    """Steps 0 and 1, the reference's two files (or the two dicts), a fresh model and trainer, ``rate_step=0`` — the reference's
    ``--resume_training``: the moments and Adam's step continue, the schedule and the sparsity-loss ramp restart — steps 2 and 3."""
    g18 = golden("g18_tiny_resume")
    build = (lambda: _masked(P)) if case in RR.G18_MASKED else (lambda: _dense(P))
    cfg, b = RR.g18_config(case), _batch()
    m = build()
    tr = _trainer(m, cfg)
    losses, rates = [], []
    _golden_steps(m, tr, b, range(RR.G18_SPLIT), losses, rates)
    m2 = build()
    tr2 = _trainer(m2, cfg)
    assert tr.optimizer_group_names() == [[str(n) for n in g18[f"{case}/group{i}_names"]] for i in range(int(g18[f"{case}/n_groups"]))]
    if via == "files":
        tr.save_checkpoint(str(tmp_path))
        assert sorted(os.listdir(tmp_path)) == ["model_last.pth", "optimizer_last.pth", "trainer_last.pth"]
        os.remove(os.path.join(str(tmp_path), "trainer_last.pth"))          # what a reference run leaves behind
        tr2.load_checkpoint(str(tmp_path), rate_step=0)
    else:
        weights = {k: v.detach().clone() for k, v in m.state_dict().items()}
        tr2.load_optimizer_state_dict(tr.optimizer_state_dict(), rate_step=0)
        m2.load_state_dict(weights, strict=False)
    assert (tr2.step_count, tr2.optim_step) == (0, 0 if tr.spec.kind == "sgd" else (1 if tr.spec.kind in ("sgdm", "sgdmom") else RR.G18_SPLIT))
    del m, tr
    _golden_steps(m2, tr2, b, range(RR.G18_SPLIT, RR.G18_STEPS), losses, rates)
    _check_case(g18, case, m2, losses, rates)


# ---------------------------------------------------------------------------------------------- 2. exact continuation, replayed gradients
@pytest.fixture(scope="module")
def recorded_grads(P):
    """The gradient arenas of four real steps, recorded once (test_gpu_optim.py::test_default_path_is_byte_equal: the backward's
    split-K atomics make two real steps differ in their last bits, everything after the backward is deterministic)."""
    from sparse_image_captioning_amd.training import NativeTrainer
    m, b = _dense(P), _batch()
    rec = NativeTrainer(m, noamopt_factor=1.0, noamopt_warmup=10, grad_clip=0.1, keep_grads=True)
    grads = []
    for _ in range(RR.G18_STEPS):
        rec.xe_step(b, train=False)
        grads.append(rec.grads.clone())
    assert all(g.abs().max().item() > 1e-3 for g in grads)
    return grads


def _replay(tr, grads):
    it = iter(grads)

    def replay(batch, norm, train=True, seed=None, after_decoder_half=None, **_):
        tr.grads.copy_(next(it))
        if after_decoder_half is not None:
            after_decoder_half()
        return 0
    tr._fwd_bwd = replay


def _snapshot(m, tr):
    torch.cuda.synchronize()
    out = {"_flat": _bytes(m._flat), "step_count": tr.step_count, "optim_step": tr.optim_step, "rate": tr.rate()}
    if getattr(m, "MASKED", False):
        out["_mask_flat"] = _bytes(m._mask_flat)
    for name in ("m", "v", "mm", "mv"):
        if getattr(tr, name, None) is not None:
            out[name] = _bytes(getattr(tr, name))
    return out


REPLAY_CASES = [(c, None) for c in R.G17_DENSE] + [("masked_step_adam", True), ("masked_step_adam", False), ("masked_cosine_rmsprop", False)]


@pytest.mark.parametrize("case,fused", REPLAY_CASES)
def test_exact_continuation_on_replayed_gradients(P, recorded_grads, tmp_path, case, fused):
    """Four replayed steps against two, ``save_checkpoint``, a fresh model and trainer, ``load_checkpoint`` and the last two: the
    weights, every state array, the mask logits and their arrays, both step counts and the rate are the same bytes.  Every kind (sgd
    included), dense on the two-stream path, masked on the one-pass tail and on the unfused one."""
    masked = fused is not None
    cfg, b = R.g17_config(case), _batch()

    def build():
        m = _masked(P) if masked else _dense(P)
        tr = _trainer(m, cfg, mask_lr=R.G17_MASK["lr_mask"][case]) if masked else _trainer(m, cfg)
        if masked:
            tr.fused_masked_tail = fused
            assert (fused and tr.spec.plain_adam) or not fused
        else:
            assert tr.early_adam
        assert recorded_grads[0].numel() == tr.grads.numel()
        return m, tr

    def steps(m, tr, which):
        _replay(tr, [recorded_grads[s] for s in which])
        for step in which:
            tr.epoch = step
            tr.xe_step(b, train=masked)

    def run(split=None, zero_state=False):
        m, tr = build()
        steps(m, tr, range(RR.G18_STEPS if split is None else split))
        if split is not None:
            tr.save_checkpoint(str(tmp_path))
            m, tr = build()
            tr.load_checkpoint(str(tmp_path))
            if zero_state:
                for name in ("m", "v", "mm", "mv"):
                    if getattr(tr, name, None) is not None:
                        getattr(tr, name).zero_()
            steps(m, tr, range(split, RR.G18_STEPS))
        assert not tr.grads.any().item()
        return _snapshot(m, tr)

    straight = run()
    assert run() == straight                                     # the replay is deterministic: the comparison below means something
    assert straight["step_count"] == straight["optim_step"] == RR.G18_STEPS
    resumed = run(split=RR.G18_SPLIT)
    assert sorted(resumed) == sorted(straight)
    assert [k for k in straight if resumed[k] != straight[k]] == []
    n_arrays = R.N_STATES["adam" if cfg["lr_scheduler"] == "noam" else cfg["optim"]]
    assert len([k for k in straight if k in ("m", "v")]) == n_arrays
    if n_arrays:                                                  # a resume that lost its state arrays ends elsewhere
        lost = run(split=RR.G18_SPLIT, zero_state=True)
        assert lost["_flat"] != straight["_flat"] and lost["step_count"] == straight["step_count"]


# ---------------------------------------------------------------------------------------------- 3. exact continuation, real steps, dropout on
def _substitute(tr, grads, trace):
    """The REAL forward, criterion and backward under the seed the step draws, then a recorded gradient in place of the backward's: the
    update, and with it the weights of the next step, are the same bytes in every run, while the loss still sees every dropout site."""
    it = iter(grads)
    real = type(tr)._fwd_bwd.__get__(tr)

    def fwd_bwd(batch, norm, train=True, seed=None, after_decoder_half=None, **kw):
        seed = real(batch, norm, train, seed, after_decoder_half=None, **kw)
        trace.append(("seed", seed))
        tr.grads.copy_(next(it))
        if after_decoder_half is not None:
            after_decoder_half()
        return seed
    tr._fwd_bwd = fwd_bwd


def _real_run(P, tmp_path, masked, save_at=None, resume=False, reset_counter=False, substitute=None, trace=None):
    """Real training-mode steps (dropout on; the supermask model samples its masks) up to step four.  Without `resume`: all four from
    torch seed 1234, writing a checkpoint after `save_at` steps and running on.  With `resume`: a model and a trainer built under
    ANOTHER torch seed load that checkpoint and take the remaining steps.  `substitute`: recorded gradients for `_substitute`; `trace`
    collects seeds and losses."""
    torch.manual_seed(4321 if resume else 1234)
    cfg, b = (R.g17_config("masked_step_adam") if masked else dict(R.G17_DEFAULTS)), _batch()          # (the defaults: noam + adam)
    m = _masked(P, dropout=True) if masked else _dense(P)
    tr = _trainer(m, cfg)
    trace = [] if trace is None else trace
    first = 0
    if resume:
        tr.load_checkpoint(str(tmp_path))
        assert m._seed_base == 1234 and m._seed_counter == RR.G18_SPLIT == tr.step_count
        if reset_counter:
            m._seed_counter = 0
        first = RR.G18_SPLIT
    which = range(first, RR.G18_STEPS)
    if substitute is not None:
        _substitute(tr, [substitute[s] for s in which], trace)
    for step in which:
        tr.epoch = step
        trace.append(("loss", tr.xe_step(b, train=True).item()))
        if save_at == step + 1:
            tr.save_checkpoint(str(tmp_path))
    torch.cuda.synchronize()
    if substitute is not None:
        trace.append(("state", _snapshot(m, tr)))
    return {n: p.detach().cpu().clone() for n, p in m.named_parameters() if not n.endswith(NOISE_ONLY)}


# The key-projection biases are left out of the distances below, as they are left out of the parameter checksums of goldens G4, G17
# and G18: softmax is invariant to a shift of a row of scores, so their true gradient is ZERO and what the backward leaves there is
# the rounding noise of its atomics (1e-9); Adam divides that noise by its own magnitude and moves each of them by about the rate per
# step in a direction that differs from run to run.  Two uninterrupted runs from one seed state lie 3e-2 apart on these biases and
# 1e-5 on everything else (measured); with them in, d0 would say nothing about the resume.
NOISE_ONLY = "attn.linears.1.bias"


def _distance(a, b):
    assert list(a) == list(b)
    return max((a[n] - b[n]).abs().max().item() for n in a)


@pytest.mark.parametrize("masked", [False, True], ids=["dense_noam_adam", "supermask"])
def test_exact_continuation_on_real_steps_with_dropout(P, tmp_path, capsys, masked):
    """Dropout (and, for the supermask model, the Bernoulli mask samples) on: every site is keyed by the seed base and counter, which
    the checkpoint carries into a process with another torch seed.

    d0 = the largest parameter difference (mask logits included, key-projection biases excluded: NOISE_ONLY above) between two
    uninterrupted four-step runs from the same seed state: the backward's atomics.  The first of them writes a checkpoint after two
    steps and runs on (if saving disturbed a run, d0 would show it: the second does not save).  The resumed run — that checkpoint
    loaded into a model and a trainer built under another torch seed, two more steps — lies within 4 x d0 of the run it continues;
    the factor covers the two runs' rounding paths diverging over two more steps.  Where d0 is 0 it is byte-equal.  The same resume
    with the seed counter reset to 0 misses that bar by at least 20 x: the test does see the seeds.

    Measured on an MI355X, 12 trials per model (profiles/resume.txt): d0 is not 0 at this size — 9.8e-7 .. 1.3e-5 dense, 6.1e-5 ..
    1.6e-4 supermask — and the resumed run lies 6e-8 .. 1.2e-7 (dense) and 9.5e-7 .. 1.4e-6 (supermask) from the run it continues, at
    most 0.12 x d0; counter reset: 4.5e-2 and 20.1.  (A resumed run that repeats the first two steps on its own instead of continuing
    run A's checkpoint is one more draw from the distribution d0 is drawn from; that distribution is wide — Adam turns the atomics'
    noise of the FIRST steps on a few near-zero-gradient elements into steps of 2e-6 .. 9e-6 that are there in one run and not in
    the next — and such a run missed 4 x d0 by chance in 28 of 224 combinations of 8 + 4 runs.)"""
    a = _real_run(P, tmp_path, masked, save_at=RR.G18_SPLIT)
    resumed = _real_run(P, tmp_path, masked, resume=True)
    wrong = _real_run(P, tmp_path, masked, resume=True, reset_counter=True)
    a2 = _real_run(P, tmp_path, masked)
    d0, dist, dist_wrong = _distance(a, a2), _distance(resumed, a), _distance(wrong, a)
    with capsys.disabled():
        print(f"\nresume on real steps, {'supermask' if masked else 'dense noam+adam'}: d0 {d0:.3e}, resumed {dist:.3e} (bar {4 * d0:.3e}), "
              f"seed counter reset {dist_wrong:.3e}")
    assert dist <= 4 * d0
    if d0 == 0.0:
        assert all(torch.equal(resumed[n], a[n]) for n in a)
    assert dist_wrong > 0 and dist_wrong >= 20 * 4 * d0


@pytest.mark.parametrize("masked", [False, True], ids=["dense_noam_adam", "supermask"])
def test_seeds_after_a_resume_on_real_forward_passes(P, recorded_grads, tmp_path, masked):
    """The property of the test above with the noise taken out: every step runs its real forward, criterion and backward with dropout
    (and mask sampling) on, and then takes a recorded gradient in place of the backward's, so that the weights are the same bytes in
    every run.  The forward and the criterion have no atomics (the loss is a fixed-order sum), so d0 IS 0 here: a run that saves on
    its way equals one that does not, and the resumed run, built under another torch seed, draws the same seeds, returns the same
    losses and ends in the same bytes as the run it continues.  With the seed counter reset to 0 it draws the first two seeds again
    and returns other losses."""
    def run(**kw):
        trace = []
        _real_run(P, tmp_path, masked, substitute=recorded_grads, trace=trace, **kw)
        return trace

    straight = run(save_at=RR.G18_SPLIT)
    resumed, wrong = run(resume=True), run(resume=True, reset_counter=True)
    assert run() == straight                                      # d0 = 0, and saving does not disturb the run
    seeds = [v for k, v in straight if k == "seed"]
    assert len(seeds) == RR.G18_STEPS == len(set(seeds))
    assert [k for k, _ in straight] == ["seed", "loss"] * RR.G18_STEPS + ["state"]
    tail = straight[2 * RR.G18_SPLIT:]
    assert [k for k, _ in resumed] == [k for k, _ in tail]
    assert [i for i, (x, y) in enumerate(zip(resumed, tail)) if x != y] == []
    assert [v for k, v in wrong if k == "seed"] == seeds[:RR.G18_SPLIT]
    losses = lambda t: [v for k, v in t if k == "loss"]
    assert all(abs(x - y) > 1e-3 for x, y in zip(losses(wrong), losses(tail)))


# ---------------------------------------------------------------------------------------------- 4. SCST
def test_scst_rollout_tokens_after_a_resume(P, recorded_grads, tmp_path):
    """One SCST step, a checkpoint, one more: the rollout of the second step draws the tokens of the uninterrupted run (the draws are
    keyed by the seed; the first step's gradient is replayed so that both runs sample from the same weights)."""
    b, ns = _batch(), 3
    cfg = dict(R.G17_DEFAULTS)                                   # noam + adam

    def reward(seq, greedy):                # device-side and synthetic: no host synchronisation, no scorer
        return (seq.reshape(-1, seq.size(-1)) % 7).float().mean(1) - 2.0

    def step(tr, replay):
        real = tr.__class__._fwd_bwd.__get__(tr)
        if replay:
            _replay(tr, [recorded_grads[0]])
        else:
            tr._fwd_bwd = real
        _, _, seq, greedy = tr.scst_step(b, reward, num_samples=ns)
        torch.cuda.synchronize()
        return seq.cpu(), greedy.cpu()

    def run(resume, reset_counter=False):
        torch.manual_seed(77)
        m = _dense(P)
        tr = _trainer(m, cfg)
        first = step(tr, True)
        if resume:
            tr.save_checkpoint(str(tmp_path))
            torch.manual_seed(5)
            m = _dense(P)
            tr = _trainer(m, cfg)
            tr.load_checkpoint(str(tmp_path))
            if reset_counter:
                m._seed_counter = 0
        return first, step(tr, False)

    (f0, s0), (f1, s1) = run(False), run(True)
    assert torch.equal(f0[0], f1[0]) and torch.equal(f0[1], f1[1])
    assert torch.equal(s0[0], s1[0]) and torch.equal(s0[1], s1[1])
    assert not torch.equal(s0[0], f0[0])                         # the second step's draws are not the first's
    _, s2 = run(True, reset_counter=True)
    assert not torch.equal(s2[0], s0[0])                         # ... and a lost counter draws other tokens


# ---------------------------------------------------------------------------------------------- 5. round trip
def _shared(P, golden):
    names = [str(n) for n in golden("g8_tiny_share_layer")["param_names"]]
    state = H.shared_layer_state(SHARE_CFG, names, C.G1_SEED, C.G1_GEN_SCALE, C.G1_EOS_BIAS)           # (every position has its keys)
    return _model(P, "relation_transformer", SHARE_CFG, state)


@pytest.mark.parametrize("which", ["dense", "supermask", "share_layer"])
def test_state_round_trip(P, golden, which):
    """``load_state_dict(state_dict())`` into a fresh trainer: every array, both counts, the epoch and the seeds.  The ACORT
    share-layer model (golden G8's config) keeps ONE entry per shared parameter."""
    build = {"dense": lambda: _dense(P), "supermask": lambda: _masked(P), "share_layer": lambda: _shared(P, golden)}[which]
    cfg = R.g17_config("masked_step_adam" if which == "supermask" else "step_adam")
    m, b = build(), _batch()
    tr = _trainer(m, cfg)
    for step in range(2):
        tr.epoch = step
        tr.xe_step(b, train=which == "supermask")
    sd = tr.state_dict()
    names = [e["name"] for e in m.named_weight_entries()]
    assert sorted(sd["state"]) == ["exp_avg", "exp_avg_sq"] and all(list(v) == names for v in sd["state"].values())
    assert all(t.device.type == "cpu" and t.dtype == torch.float32 for v in sd["state"].values() for t in v.values())
    assert all(tuple(sd["state"]["exp_avg"][e["name"]].shape) == tuple(e["shape"]) for e in m.named_weight_entries())
    assert sd["format"] == 1 and (sd["rate_step"], sd["optim_step"], sd["epoch"]) == (2, 2, 1)
    if which == "share_layer":
        keys = [k for k in m.state_dict() if not k.endswith(".pe")]
        assert len(names) < len(keys) and set(names) < set(keys)              # state_dict lists every position, the state each tensor once
        assert not any(n.startswith(("model.encoder.layers.2.", "model.decoder.layers.1.")) for n in names)
    if which == "supermask":
        assert all(n.endswith("_pruning_mask") for v in sd["mask_state"].values() for n in v) and sd["mask_state"]["exp_avg"]
    else:
        assert "mask_state" not in sd
    m2 = build()
    tr2 = _trainer(m2, cfg)
    tr2.load_state_dict(sd)
    torch.cuda.synchronize()
    for name in ("m", "v", "mm", "mv"):
        if getattr(tr, name, None) is not None:
            assert torch.equal(getattr(tr, name), getattr(tr2, name)), name
            assert getattr(tr, name).any().item(), name
    assert (tr2.step_count, tr2.optim_step, tr2.epoch) == (2, 2, 1)
    assert (m2._seed_base, m2._seed_counter) == (torch.initial_seed(), m._seed_counter)
    assert not tr2.grads.any().item()
    # the reference's format carries the same arrays: through it and back
    tr3 = _trainer(build(), cfg)
    tr3.load_optimizer_state_dict(tr.optimizer_state_dict())
    assert (tr3.step_count, tr3.optim_step) == (2, 2)
    for name in ("m", "v", "mm", "mv"):
        if getattr(tr, name, None) is not None:
            assert torch.equal(getattr(tr, name), getattr(tr3, name)), name
