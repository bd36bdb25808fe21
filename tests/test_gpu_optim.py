"""The optimiser family on the device: ``ortk_optim_step`` against the numpy fp32 restatement (tests/optim_ref.py), its shapes,
switches and refusals, and ``NativeTrainer`` with the reference's optimiser options end to end against golden G17 (the reference's own
runs, tests/golden/make_golden_optim.py).  The default trainer must stay the parent's bytes."""
import ctypes as Ct
import zlib

import numpy as np
import pytest
import torch

import common as C
import helpers as H
import optim_ref as R

pytestmark = pytest.mark.gpu

# 4 x the distance the host test measured between the restatement and torch.optim at the same inputs (test_optim_host.py): the factor
# covers fused multiply-adds and the device's division and square-root rounding
BAR = 4 * R.HOST_DISTANCE


@pytest.fixture(scope="module")
def P():
    import sparse_image_captioning_amd as pkg
    pkg._lib.require_gpu()
    return pkg


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _args(P, kind, p, g, state, t=1, lr=0.1, alpha=0.875, beta=0.99609375, eps=1e-8, wd=0.0, clip=R.OP_CLIP, zero=False, first=None):
    L = P._lib
    k = L.OptimArgs()
    k.p, k.g, k.n = p.data_ptr(), g.data_ptr(), p.numel()
    k.s1 = state[0].data_ptr() if len(state) >= 1 else None
    k.s2 = state[1].data_ptr() if len(state) >= 2 else None
    k.kind, k.first_step, k.zero_grad = L.OPT_KINDS[kind], int(t == 1 if first is None else first), int(zero)
    k.lr, k.weight_decay, k.alpha, k.beta, k.eps, k.clip = lr, wd, alpha, beta, eps, clip
    k.bc1, k.bc2 = 1.0 - alpha ** t, 1.0 - beta ** t
    return k


def _call(P, k):
    return P._lib.lib().ortk_optim_step(Ct.byref(k), P._lib.stream_ptr())


def _step(P, kind, p, g, state, **kw):
    assert _call(P, _args(P, kind, p, g, state, **kw)) == 0
    torch.cuda.synchronize()


def _new_state(kind, n):
    return [torch.zeros(n, device="cuda") for _ in range(R.N_STATES[kind])]


def test_state_array_counts(P):
    lib = P._lib.lib()
    assert [lib.ortk_optim_states(P._lib.OPT_KINDS[k]) for k in R.KINDS] == [R.N_STATES[k] for k in R.KINDS]
    assert lib.ortk_optim_states(6) == -1 and lib.ortk_optim_states(-1) == -1


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("kind", R.KINDS)
def test_operator_vs_restatement(P, kind, wd, capsys):
    """6 steps at the host test's inputs (n = 4099: vector body plus a 3-element tail), parameters and state arrays."""
    lr, alpha, beta, eps = R.OP_HYPER[kind]
    p0, grads = R.op_inputs()
    ref, rstate = p0.copy(), R.new_state(kind, p0.size)
    p, state = _dev(p0), _new_state(kind, p0.size)
    for t, g in enumerate(grads, 1):
        R.step(kind, ref, g, rstate, t, lr, alpha, beta, eps, wd, R.OP_CLIP)
        _step(P, kind, p, _dev(g), state, t=t, lr=lr, alpha=alpha, beta=beta, eps=eps, wd=wd)
    dist = float(np.abs(p.cpu().numpy() - ref).max())
    with capsys.disabled():
        print(f"\nortk_optim_step vs restatement: {kind:8s} weight_decay {wd:g}: max |diff| {dist:.3e} (bar {BAR:.3e})")
    assert float(np.abs(ref - p0).max()) > 1e-2              # the run moved the parameters by far more than the bar
    assert dist <= BAR
    for s, r in zip(state, rstate):                          # the state arrays carry the same rule
        np.testing.assert_allclose(s.cpu().numpy(), r, rtol=1e-5, atol=BAR)


def test_shapes_tail_only_empty_and_a_range_with_neighbours(P):
    rs = np.random.RandomState(5)
    for kind in R.KINDS:
        lr, alpha, beta, eps = R.OP_HYPER[kind]
        kw = dict(lr=lr, alpha=alpha, beta=beta, eps=eps, wd=1e-2)
        # n = 3: tail only
        p0, g0 = (0.1 * rs.standard_normal(3)).astype(np.float32), (0.3 * rs.standard_normal(3)).astype(np.float32)
        ref, rstate = p0.copy(), R.new_state(kind, 3)
        R.step(kind, ref, g0, rstate, 1, lr, alpha, beta, eps, 1e-2, R.OP_CLIP)
        p, state = _dev(p0), _new_state(kind, 3)
        _step(P, kind, p, _dev(g0), state, **kw)
        assert float(np.abs(p.cpu().numpy() - ref).max()) <= BAR, kind
        # n = 0: returns 0 and touches nothing
        before = p.clone()
        k = _args(P, kind, p, _dev(g0), state, **kw)
        k.n = 0
        assert _call(P, k) == 0
        torch.cuda.synchronize()
        assert torch.equal(p, before)
        # 1021 elements starting at element 4 of a larger buffer: the neighbours stay byte-unchanged
        N, a, n = 1100, 4, 1021
        big = [(0.1 * rs.standard_normal(N)).astype(np.float32) for _ in range(2 + R.N_STATES[kind])]
        big[2:] = [np.abs(b) for b in big[2:]]                                       # (second moments are non-negative)
        dev = [_dev(b) for b in big]
        ref, rstate = big[0][a:a + n].copy(), [b[a:a + n].copy() for b in big[2:]]
        R.step(kind, ref, big[1][a:a + n].copy(), rstate, 2, lr, alpha, beta, eps, 1e-2, R.OP_CLIP)
        _step(P, kind, dev[0][a:a + n], dev[1][a:a + n], [d[a:a + n] for d in dev[2:]], t=2, zero=True, **kw)
        got = [d.cpu().numpy() for d in dev]
        assert float(np.abs(got[0][a:a + n] - ref).max()) <= BAR, kind
        assert not got[1][a:a + n].any()
        for b, o in zip(big, got):
            assert b[:a].tobytes() == o[:a].tobytes() and b[a + n:].tobytes() == o[a + n:].tobytes(), kind


def test_grid_stride_loop_runs_more_than_once(P):
    """n = 4 200 003: more than the 4 096 x 256 lanes x 4 elements one sweep of the grid covers, plus a tail (adam with decay)."""
    n = 4_200_003
    rs = np.random.RandomState(11)
    p0 = (0.1 * rs.standard_normal(n)).astype(np.float32)
    lr, alpha, beta, eps = R.OP_HYPER["adam"]
    ref, rstate = p0.copy(), R.new_state("adam", n)
    p, state = _dev(p0), _new_state("adam", n)
    for t in (1, 2):
        g = ((0.3 if t == 1 else 0.02) * rs.standard_normal(n)).astype(np.float32)
        R.step("adam", ref, g, rstate, t, lr, alpha, beta, eps, 1e-2, R.OP_CLIP)
        gd = _dev(g)
        _step(P, "adam", p, gd, state, t=t, lr=lr, alpha=alpha, beta=beta, eps=eps, wd=1e-2, zero=True)
        assert not gd.any().item()
    got = p.cpu().numpy()
    assert float(np.abs(got - ref).max()) <= BAR
    assert float(np.abs(got - p0).min()) > 0.0               # every element was visited


def test_switches(P):
    rs = np.random.RandomState(3)
    n = 4099
    p0, g0, b0 = [(0.1 * rs.standard_normal(n)).astype(np.float32) for _ in range(3)]
    # zero_grad clears g; without it g is intact
    for kind in R.KINDS:
        g = _dev(g0)
        _step(P, kind, _dev(p0), g, _new_state(kind, n), zero=False)
        assert g.cpu().numpy().tobytes() == g0.tobytes(), kind
        _step(P, kind, _dev(p0), g, _new_state(kind, n), zero=True)
        assert not g.any().item(), kind
    # the first-step flag of the momentum kinds: the buffer is overwritten (first) or continued (later), whatever it holds
    for kind in ("sgdm", "sgdmom"):
        for first in (True, False):
            ref, rbuf = p0.copy(), [b0.copy()]
            R.step(kind, ref, g0, rbuf, 5, 0.2, 0.875, clip=R.OP_CLIP, first_step=first)
            p, buf = _dev(p0), [_dev(b0)]
            _step(P, kind, p, _dev(g0), buf, t=5, lr=0.2, first=first)
            assert float(np.abs(p.cpu().numpy() - ref).max()) <= BAR and float(np.abs(buf[0].cpu().numpy() - rbuf[0]).max()) <= BAR
        a, b = [], []
        for first, out in ((True, a), (False, b)):
            p = _dev(p0)
            _step(P, kind, p, _dev(g0), [_dev(b0)], t=5, lr=0.2, first=first)
            out.append(p.cpu().numpy())
        assert float(np.abs(a[0] - b[0]).max()) > 1e-3        # the flag matters
    # two runs give the same bytes
    for kind in R.KINDS:
        outs = []
        for _ in range(2):
            p, state = _dev(p0), _new_state(kind, n)
            for t in (1, 2):
                _step(P, kind, p, _dev(g0), state, t=t, wd=1e-2)
            outs.append(p.cpu().numpy().tobytes() + b"".join(s.cpu().numpy().tobytes() for s in state))
        assert outs[0] == outs[1], kind
    # sgd never touches a state pointer: null is fine
    k = _args(P, "sgd", _dev(p0), _dev(g0), [])
    assert k.s1 is None and k.s2 is None and _call(P, k) == 0
    torch.cuda.synchronize()


def test_refusals(P):
    """Every refusal of include/ortk.h returns ORTK_EINVAL (-1) before any launch: the parameters stay as they were."""
    n = 64
    p, g = torch.zeros(n, device="cuda"), torch.ones(n, device="cuda")
    s = [torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    lib = P._lib.lib()
    inf, nan = float("inf"), float("nan")

    def bad(opt="adam", **field):
        k = _args(P, opt, p, g, s[:R.N_STATES[opt]])
        for name, v in field.items():
            setattr(k, name, v)
        return _call(P, k)

    assert bad() == 0 and bad(clip=inf) == 0                       # the unperturbed call is accepted; +inf = no clipping
    p.zero_()
    codes = {
        "null args": lib.ortk_optim_step(None, P._lib.stream_ptr()),
        "null p": bad(p=None), "null g": bad(g=None),
        "null s1 (adam)": bad(s1=None), "null s2 (adam)": bad(s2=None),
        "null s1 (sgdm)": bad("sgdm", s1=None), "null s1 (sgdmom)": bad("sgdmom", s1=None),
        "null s1 (rmsprop)": bad("rmsprop", s1=None), "null s1 (adagrad)": bad("adagrad", s1=None),
        "n < 0": bad(n=-1), "kind 6": bad(kind=6), "kind -1": bad(kind=-1),
        "misaligned p": bad(p=p.data_ptr() + 4), "misaligned g": bad(g=g.data_ptr() + 4),
        "misaligned s1": bad(s1=s[0].data_ptr() + 8), "misaligned s2": bad(s2=s[1].data_ptr() + 4),
        "clip 0": bad(clip=0.0), "clip < 0": bad(clip=-0.1), "clip nan": bad(clip=nan),
        "lr inf": bad(lr=inf), "lr nan": bad(lr=nan), "weight_decay nan": bad(weight_decay=nan), "weight_decay inf": bad(weight_decay=-inf),
        "alpha nan": bad(alpha=nan), "beta inf": bad(beta=inf), "eps nan": bad(eps=nan), "eps inf": bad("rmsprop", eps=inf),
        "bc1 0": bad(bc1=0.0), "bc2 0": bad(bc2=0.0), "bc1 < 0": bad(bc1=-0.5), "bc2 nan": bad(bc2=nan),
    }
    torch.cuda.synchronize()
    assert all(c == -1 for c in codes.values()), {k: c for k, c in codes.items() if c != -1}
    assert not p.any().item()
    assert bad("sgd", s1=None, s2=None, bc1=0.0, bc2=0.0) == 0      # bc1 / bc2 are adam's; sgd has no state
    assert bad(n=0, lr=0.5) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the trainer, end to end
def _model(P, name, cfg, state, **over):
    from sparse_image_captioning_amd.utils.config import Config
    m = P.get_model(name)(Config(**dict(cfg, **over)))
    missing, unexpected = m.load_state_dict(state, strict=False)
    assert not unexpected and all(k.endswith(".pe") or k.endswith("_pruning_mask") for k in missing), (missing, unexpected)
    return m.cuda().eval()


def _batch():
    return {k: v.cuda() for k, v in H.g1_batch().items()}


def _check_case(g17, case, m, losses, rates):
    """The bars of test_native_trainer_noam_adam_clip_vs_reference_golden: losses 5e-4, rates 1e-12, parameters 5e-4, checksum 1e-4."""
    np.testing.assert_allclose(rates, g17[f"{case}/rates"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(losses, g17[f"{case}/losses"], rtol=0, atol=5e-4)
    sd = {n: p.detach().cpu().numpy() for n, p in m.named_parameters()}
    n_checked = 0
    for k, v in g17.items():
        if k.startswith(f"{case}/param/"):
            name = k[len(case) + 7:]
            if name.endswith("_pruning_mask"):
                # a mask logit moves by lr_mask * O(1) per step on 1e-7 gradient noise: the bar golden G13 is held to
                # (test_supermask_train_mode_and_mask_optimizer_vs_reference_golden)
                np.testing.assert_allclose(sd[name], v, rtol=2e-3, atol=5e-2, err_msg=k)
            else:
                np.testing.assert_allclose(sd[name], v, rtol=0, atol=5e-4, err_msg=k)
            n_checked += 1
    assert n_checked >= 4
    tot = sum(float(np.abs(v.astype(np.float64)).sum()) for n, v in sd.items() if not n.endswith("attn.linears.1.bias"))
    assert abs(tot - float(g17[f"{case}/param_abs_sum"])) / tot < 1e-4


@pytest.mark.parametrize("case", list(R.G17_DENSE))
def test_trainer_dense_vs_reference_golden(P, golden, case):
    """3 x xe_step(train=False) with the case's optimiser options, `epoch` set as the generator passed it to opt.step(epoch=step)."""
    from sparse_image_captioning_amd.training import NativeTrainer
    g17 = golden("g17_tiny_optim_family")
    m, b = _model(P, "relation_transformer", C.TINY_CFG, H.g1_state()), _batch()
    tr = NativeTrainer(m, grad_clip=R.G17_CLIP, **R.g17_config(case))
    kind = tr.spec.kind
    assert (tr.m is not None, tr.v is not None) == (R.N_STATES[kind] >= 1, R.N_STATES[kind] >= 2)       # only the state the kind needs
    losses, rates = [], []
    for step in range(R.G17_STEPS):
        tr.epoch = step
        losses.append(tr.xe_step(b, train=False).item())
        rates.append(tr.rate())
    _check_case(g17, case, m, losses, rates)


@pytest.mark.parametrize("case,fused", [("masked_step_adam", True), ("masked_step_adam", False), ("masked_cosine_rmsprop", False)])
def test_trainer_masked_vs_reference_golden(P, golden, case, fused):
    """The supermask model with the reference's two param groups: weights under the scheduled optimiser, the ACTIVE mask logits under
    the same kind at lr = prune_supermask_lr, eps 1e-2, no weight decay, no scheduler.  Adam without weight decay takes the fused tail
    (ortk_masked_adam_step) at the scheduled rate and, with `fused_masked_tail` off, the unfused one; rmsprop has the unfused tail only."""
    from sparse_image_captioning_amd.training import NativeTrainer
    g17 = golden("g17_tiny_optim_family")
    shapes = H.prune_param_shapes(C.TINY_CFG)
    mask_shapes = {k: v for k, v in shapes.items() if k.endswith("_pruning_mask")}
    state = H.torch_state(shapes, C.G1_SEED, C.G1_GEN_SCALE, C.G1_EOS_BIAS, keep_prob=C.G3_KEEP)
    m = _model(P, "relation_transformer_prune", C.TINY_CFG, state, prune_mask_freeze_scope="model.generator.", prune_supermask_init=5.0)
    m.train()
    m._ccfg.drop, m._ccfg.drop_src = 0.0, 0.0
    frozen0 = {n: p.detach().clone() for n, p in m.all_pruning_masks() if n.startswith("model.generator.")}
    M = R.G17_MASK
    tr = NativeTrainer(m, grad_clip=R.G17_CLIP, prune_supermask_lr=M["lr_mask"][case], mask_eps=1e-2, sparsity_target=M["target"],
                       sparsity_weight=M["weight"], **R.g17_config(case))
    assert tr.spec.plain_adam == (case == "masked_step_adam")
    tr.fused_masked_tail = fused
    u = lambda shape, step: np.random.RandomState((zlib.crc32(str(tuple(shape)).encode()) + 7919 * step) & 0x7FFFFFFF).uniform(
        size=tuple(shape)).astype(np.float32)
    b = _batch()
    losses, rates = [], []
    for step in range(R.G17_STEPS):
        tr.epoch = step
        m.set_mask_draws({k: u(shp, step) for k, shp in mask_shapes.items()})
        losses.append(tr.xe_step(b).item())
        rates.append(tr.rate())
    _check_case(g17, case, m, losses, rates)
    for n, p0 in frozen0.items():                              # frozen scope: bit-unchanged under every kind
        assert torch.equal(dict(m.all_pruning_masks())[n].detach(), p0), n
    tot = sum(p.detach().double().abs().sum().item() for _, p in m.all_pruning_masks())
    assert abs(tot - float(g17[f"{case}/mask_abs_sum"])) / float(g17[f"{case}/mask_abs_sum"]) < 2e-3          # (G13's bar)


def test_default_path_is_byte_equal(P):
    """Adam without weight decay keeps the kernel and the arguments it has always had: the step schedule at Noam's first rate gives
    the default trainer's bytes after one step, and the default trainer equals optim="adam", lr_scheduler="noam" after three.

    The backward's split-K atomics make the gradient differ in its last bits from run to run (test_gpu_model.py: "equal up to
    rounding, not bitwise"), so two independent steps can never be compared byte for byte.  The gradients of three real steps are
    therefore recorded once and replayed into every trainer in place of its forward + backward; everything after the backward — the
    rate, the two-stream split, the dispatcher, the kernel and its arguments — runs as in a real step and IS deterministic."""
    from sparse_image_captioning_amd.training import NativeTrainer, noam_rate
    b = _batch()
    m = _model(P, "relation_transformer", C.TINY_CFG, H.g1_state())
    rec = NativeTrainer(m, noamopt_factor=1.0, noamopt_warmup=10, grad_clip=0.1, keep_grads=True)
    grads = []
    for _ in range(3):
        rec.xe_step(b, train=False)
        grads.append(rec.grads.clone())
    assert all(g.abs().max().item() > 1e-3 for g in grads)

    def run(steps, **kw):
        m = _model(P, "relation_transformer", C.TINY_CFG, H.g1_state())
        tr = NativeTrainer(m, noamopt_factor=1.0, noamopt_warmup=10, grad_clip=0.1, **kw)
        assert tr.early_adam                       # the production path: decoder half on the second stream, gradient cleared on the way
        it = iter(grads)

        def replay(batch, norm, train=True, seed=None, after_decoder_half=None, **_):
            tr.grads.copy_(next(it))
            if after_decoder_half is not None:
                after_decoder_half()
            return 0
        tr._fwd_bwd = replay
        for _ in range(steps):
            tr.xe_step(b, train=False)
        torch.cuda.synchronize()
        assert not tr.grads.any().item()
        return m._flat.detach().cpu().numpy().tobytes(), tr

    ref1, tr0 = run(1)
    assert tr0.spec.plain_adam and tr0.spec.scheduler == "noam"
    assert run(1)[0] == ref1                       # the replay is deterministic: the comparison below means something
    lr1 = noam_rate(1, C.TINY_CFG["d_model"], 1.0, 10)
    got1, tr1 = run(1, lr_scheduler="step", optim="adam", optim_alpha=0.9, optim_beta=0.98, optim_epsilon=1e-9, weight_decay=0,
                    learning_rate=lr1)
    assert tr1.rate() == lr1 and got1 == ref1
    ref3, _ = run(3)
    got3, _ = run(3, optim="adam", lr_scheduler="noam")
    assert got3 == ref3 and ref3 != ref1
    # a different optimiser on the same gradients does move the bytes (the comparison can fail)
    assert run(1, lr_scheduler="step", optim="adam", optim_alpha=0.9, optim_beta=0.98, optim_epsilon=1e-9, weight_decay=1e-2, learning_rate=lr1)[0] != ref1
