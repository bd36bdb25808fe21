"""The label-smoothed criterion of the native XE step (``ortk_xent_smooth_fwd_bwd`` / ``ortk_loss_smooth`` /
``NativeTrainer(label_smoothing=...)``) on a real MI355X: the operator against the fp64 closed form of the reference's
``LabelSmoothing`` (utils/losses.py:46-77, pinned by golden G7), the trainer against the oracle, a masked model and the full
vocabulary in both precisions against the criterion applied to the model's own materialised log-probs."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import common as Cm
import helpers as H
from oracle import ort_oracle as O

pytestmark = pytest.mark.gpu

R, T = 4, 6                     # 24 rows, targets in a (R, T + 1) token matrix read from column 1 on
ROWS = R * T
F32, BF16 = 0, 1
# V, ld, gradient dtype: every kernel form and both edges of the register form (2048 < V <= 10240 and ld <= 10240)
CASES = [(101, 128, F32),       # generic
         (2048, 2048, F32),     # generic, lower edge
         (2049, 2176, F32),     # register, lower edge
         (10001, 10112, F32),   # register, exact
         (10001, 10112, BF16),  # register, fast
         (10240, 10240, F32),   # register, upper edge
         (10241, 10368, F32),   # generic again
         (10001, 10368, F32)]   # V inside the register range, ld above it: generic (the register form would leave columns unwritten)
CASE_IDS = [f"V{v}-ld{ld}-{'bf16' if dt else 'f32'}" for v, ld, dt in CASES]
ROW_BAR = dict(rtol=1e-5, atol=1e-7)            # test_embed_xent_softmax_colsum's bars
GRAD_BAR = {F32: dict(rtol=1e-4, atol=1e-7),
            BF16: dict(rtol=2.0 ** -8, atol=1e-9)}      # one bf16 ulp: twice the rounding half-ulp


@pytest.fixture(scope="module")
def L():
    import sparse_image_captioning_amd as P
    P._lib.require_gpu()
    return P._lib


@functools.lru_cache(maxsize=None)
def _inputs(V, ld):
    """Logits 4 * randn over all ld columns (the pad columns hold values the kernel must not read into the result), targets that
    include columns 0 and V - 1, weights with exact zeros and non-unit values, norm = sum(w)."""
    g = torch.Generator().manual_seed(1000 + V)
    logits = (4.0 * torch.randn(ROWS, ld, generator=g)).float()
    seq = torch.randint(0, V, (R, T + 1), generator=g)
    seq[0, 1], seq[1, 2] = 0, V - 1
    w = (0.25 + 1.5 * torch.rand(ROWS, generator=g)).float()
    w[[3, 10, 23]] = 0.0
    w[5] = 1.0
    return logits, seq, w, float(w.double().sum())


@functools.lru_cache(maxsize=None)
def _reference(V, ld, eps32):
    """fp64 closed form on the CPU from the same logits, for the smoothing the C ABI received (a float):
    KL = K0 - c lp[t] - s (sum_v lp[v] - lp[t]), K0 = c ln c + (V - 1) s ln s; dKL/dz = p - q."""
    logits, seq, w, norm = _inputs(V, ld)
    lp = torch.log_softmax(logits[:, :V].double(), -1)
    tgt = seq[:, 1:].reshape(-1)
    c, s = 1.0 - eps32, eps32 / (V - 1)
    xlogx = lambda p: p * math.log(p) if p > 0 else 0.0
    lpt = lp.gather(1, tgt[:, None]).squeeze(1)
    wn = w.double() / norm
    rows = (xlogx(c) + (V - 1) * xlogx(s) - c * lpt - s * (lp.sum(1) - lpt)) * wn
    q = torch.full_like(lp, s).scatter_(1, tgt[:, None], c)
    grad = (lp.exp() - q) * wn[:, None]
    return rows, grad


def _run(L, V, ld, dt, eps, alias=False, plain=False):
    logits, seq, w, norm = _inputs(V, ld)
    lib = L.lib()
    lg, seqd, wd = logits.cuda(), seq.cuda(), w.cuda()
    nd = torch.tensor([norm], device="cuda", dtype=torch.float32)
    loss = torch.full((1,), 7.0, device="cuda")
    row_loss = torch.full((lib.ortk_xent_scratch_floats(ROWS),), float("nan"), device="cuda")
    out = lg if alias else torch.full((ROWS, ld), float("nan"), device="cuda", dtype=torch.bfloat16 if dt == BF16 else torch.float32)
    args = [L.ptr(lg), C.c_void_p(seqd.data_ptr() + 8), T + 1, T, L.ptr(wd), L.ptr(nd), L.ptr(loss), L.ptr(row_loss), ROWS, V, ld,
            L.ptr(out), dt, ld]
    if plain:
        L.check(lib.ortk_xent_fwd_bwd(*args, L.stream_ptr()), "ortk_xent_fwd_bwd")
    else:
        L.check(lib.ortk_xent_smooth_fwd_bwd(*args, eps, L.stream_ptr()), "ortk_xent_smooth_fwd_bwd")
    torch.cuda.synchronize()
    return loss.cpu(), row_loss[:ROWS].cpu(), out.cpu()


@pytest.mark.parametrize("eps", [0.1, 0.3])
@pytest.mark.parametrize("V,ld,dt", CASES, ids=CASE_IDS)
def test_smoothed_operator_vs_fp64_closed_form(L, V, ld, dt, eps):
    _, _, w, norm = _inputs(V, ld)
    ref_rows, ref_grad = _reference(V, ld, float(np.float32(eps)))
    loss, rows, out = _run(L, V, ld, dt, eps)
    err_rows = ((rows.double() - ref_rows).abs() / ref_rows.abs().clamp(min=1e-30)).max().item()
    err_grad = ((out[:, :V].double() - ref_grad).abs() / ref_grad.abs().clamp(min=1e-30))[ref_grad.abs() > 1e-6].max().item()
    print(f"V {V} ld {ld} dt {dt} eps {eps}: loss {loss.item():.8f} ref {ref_rows.sum().item():.8f} "
          f"max rel row err {err_rows:.3e} max rel grad err (|g| > 1e-6) {err_grad:.3e}")
    torch.testing.assert_close(rows.double(), ref_rows, **ROW_BAR)
    torch.testing.assert_close(loss.double(), ref_rows.sum().reshape(1), **ROW_BAR)
    torch.testing.assert_close(out[:, :V].double(), ref_grad, **GRAD_BAR[dt])
    if ld > V:
        assert float(out[:, V:].float().abs().max()) == 0.0                    # padded columns: exactly 0 (and written: not NaN)
    zero = w == 0
    assert float(out[zero].float().abs().max()) == 0.0 and float(rows[zero].abs().max()) == 0.0
    if dt == F32:
        wn = w.double() / norm
        assert bool((out[:, :V].double().sum(1).abs() <= V * 2.0 ** -24 * wn).all()), (out[:, :V].double().sum(1).abs() / wn).max()
        # dlogits aliasing logits (what the fp32 training workspace does): the same bits
        loss_a, rows_a, out_a = _run(L, V, ld, dt, eps, alias=True)
        assert torch.equal(out_a, out) and torch.equal(rows_a, rows) and torch.equal(loss_a, loss)
    loss2, rows2, out2 = _run(L, V, ld, dt, eps)                                # no atomics: a rerun gives the same bits
    assert torch.equal(out2, out) and torch.equal(rows2, rows) and torch.equal(loss2, loss)


@pytest.mark.parametrize("V,ld,dt", CASES, ids=CASE_IDS)
def test_zero_smoothing_is_the_plain_cross_entropy(L, V, ld, dt):
    loss, rows, out = _run(L, V, ld, dt, 0.0)
    loss_p, rows_p, out_p = _run(L, V, ld, dt, 0.0, plain=True)
    torch.testing.assert_close(rows, rows_p, **ROW_BAR)
    torch.testing.assert_close(loss, loss_p, **ROW_BAR)
    torch.testing.assert_close(out.float(), out_p.float(), **GRAD_BAR[dt])


def test_smoothed_operator_refuses_bad_arguments(L):
    V, ld = 101, 128
    logits, seq, w, norm = _inputs(V, ld)
    lib = L.lib()
    lg, seqd, wd = logits.cuda(), seq.cuda(), w.cuda()
    nd = torch.tensor([norm], device="cuda")
    loss = torch.zeros(1, device="cuda")
    row_loss = torch.zeros(lib.ortk_xent_scratch_floats(ROWS), device="cuda")
    out = torch.zeros(ROWS, ld, device="cuda")

    def call(eps=0.1, V=V, ld=ld, dt=F32, ld_dl=ld, T_=T, logits_=lg, rows=ROWS):
        return lib.ortk_xent_smooth_fwd_bwd(L.ptr(logits_), C.c_void_p(seqd.data_ptr() + 8), T + 1, T_, L.ptr(wd), L.ptr(nd), L.ptr(loss),
                                            L.ptr(row_loss), rows, V, ld, L.ptr(out), dt, ld_dl, eps, L.stream_ptr())
    assert call() == 0 and call(eps=0.0) == 0
    for bad in (float("nan"), float("inf"), -float("inf"), -0.1, 1.0, 1.5):
        assert call(eps=bad) == -1, bad                      # ORTK_EINVAL
    assert call(V=1) == -1                                   # V - 1 = 0 columns to spread the smoothing over
    # ... and what ortk_xent_fwd_bwd refuses
    assert call(V=0) == -1 and call(ld=V - 1) == -1 and call(ld_dl=V - 1) == -1 and call(dt=2) == -1 and call(T_=0) == -1
    assert call(rows=-1) == -1 and call(logits_=None) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ trainer
@pytest.fixture(scope="module")
def P():
    import sparse_image_captioning_amd as pkg
    pkg._lib.require_gpu()
    return pkg


def _model(P, name, cfg, state, precision=0):
    from sparse_image_captioning_amd.utils.config import Config
    m = P.get_model(name)(Config(**cfg), precision=precision)
    missing, unexpected = m.load_state_dict(state, strict=False)
    assert not unexpected and all(k.endswith(".pe") or k.endswith("_pruning_mask") for k in missing), (missing, unexpected)
    return m.cuda().eval()


def _cuda(b):
    return {k: v.cuda() for k, v in b.items()}


def _criterion_on_logp(m, b, eps):
    """LabelSmoothing on the log-probs the model materialises (eval mode)."""
    from sparse_image_captioning_amd.utils.losses import LabelSmoothing
    with torch.no_grad():
        logp = m(att_feats=b["att_feats"], boxes=b["boxes"], seqs=b["seqs"], att_masks=b["att_masks"])
        return LabelSmoothing(smoothing=eps)(logp.float(), b["seqs"][:, 1:], b["masks"][:, 1:]).item()


def test_smoothed_native_step_vs_oracle(P):
    from sparse_image_captioning_amd.training import NativeTrainer
    from sparse_image_captioning_amd.utils.losses import LabelSmoothing
    m, cb = _model(P, "relation_transformer", Cm.TINY_CFG, H.g1_state()), H.g1_batch()
    b = _cuda(cb)
    cfg = O.OCfg(**{k: v for k, v in Cm.TINY_CFG.items() if not k.startswith("prune")})
    Pm = {k: v.clone().requires_grad_() for k, v in H.g1_state().items()}
    logp = O.forward_logp(Pm, cfg, cb["att_feats"], cb["boxes"], cb["seqs"], cb["att_masks"])
    ref_loss = LabelSmoothing(smoothing=0.1)(logp, cb["seqs"][:, 1:], cb["masks"][:, 1:])
    ref_loss.backward()
    tr = NativeTrainer(m, label_smoothing=0.1, noamopt_factor=0.0, keep_grads=True)
    loss = tr.xe_step(b, train=False)
    print(f"smoothed loss {loss.item():.7f} oracle {ref_loss.item():.7f}")
    assert abs(loss.item() - ref_loss.item()) < 1e-4, (loss.item(), ref_loss.item())          # the north-star bar
    plain = O.xe_loss(logp.detach(), cb["seqs"][:, 1:], cb["masks"][:, 1:]).item()
    assert abs(ref_loss.item() - plain) > 1e-2                                                  # (another criterion, not a relabelled one)
    for e in m.named_weight_entries():
        if e["name"] in ("att_embed.0.weight", "model.decoder.layers.1.feed_forward.w_1.weight", "model.generator.proj.bias",
                         "model.encoder.layers.0.self_attn.WGs.3.weight", "model.tgt_embed.0.lut.weight"):
            got = tr.grads[e["offset"]:e["offset"] + e["numel"]].view(e["shape"]).cpu()
            ref = Pm[e["name"]].grad
            tol = 2e-4 * max(1.0, float(ref.abs().max()))
            assert (got - ref).abs().max().item() <= tol, e["name"]
    # smoothing 0 is the step a trainer built without the argument runs
    l0 = NativeTrainer(m, label_smoothing=0.0, noamopt_factor=0.0, keep_grads=True).xe_step(b, train=False)
    ld = NativeTrainer(m, noamopt_factor=0.0, keep_grads=True).xe_step(b, train=False)
    assert torch.equal(l0, ld), (l0.item(), ld.item())
    assert abs(ld.item() - plain) < 1e-4
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            NativeTrainer(m, label_smoothing=bad)


def test_smoothed_native_step_on_a_masked_model(P):
    from sparse_image_captioning_amd.training import NativeTrainer
    state = H.torch_state(H.prune_param_shapes(Cm.TINY_CFG), Cm.G1_SEED, Cm.G1_GEN_SCALE, Cm.G1_EOS_BIAS, keep_prob=Cm.G3_KEEP)
    m, b = _model(P, "relation_transformer_prune", Cm.TINY_CFG, state), _cuda(H.g1_batch())
    ref = _criterion_on_logp(m, b, 0.1)
    tr = NativeTrainer(m, label_smoothing=0.1, noamopt_factor=0.0, prune_supermask_lr=0.0)
    loss = tr.xe_step(b, train=False).item()
    print(f"masked model: smoothed loss {loss:.7f} criterion on log-probs {ref:.7f}")
    assert abs(loss - ref) < 1e-4, (loss, ref)


@pytest.fixture(scope="module")
def full_state():
    return H.torch_state(H.dense_param_shapes(Cm.FULL_CFG), Cm.G2_SEED)


def _cap_len(masks):
    w = masks[:, 1:]
    idx = torch.arange(1, w.size(1) + 1, device=w.device)
    return ((w != 0).long() * idx).max(1).values.clamp(min=1).cpu()


@pytest.mark.parametrize("precision", [0, 1])
def test_smoothed_native_step_at_full_vocabulary(P, full_state, precision):
    """FULL_CFG (V = 10001: the register-resident kernels, exact in fp32 and fast in mixed precision) on the G2 geometry."""
    from sparse_image_captioning_amd.training import NativeTrainer
    m = _model(P, "relation_transformer", Cm.FULL_CFG, full_state, precision=precision)
    b = _cuda(H.torch_batch(Cm.make_inputs(**Cm.G2_INPUTS)))
    ref = _criterion_on_logp(m, b, 0.1)
    tr = NativeTrainer(m, label_smoothing=0.1, noamopt_factor=0.0, keep_grads=True)

    def step(data):
        tr.m.zero_(); tr.v.zero_(); tr.step_count = 0
        return tr.xe_step(data, train=False).item(), tr.grads.clone()

    lp, gp = step(b)
    print(f"precision {precision}: smoothed loss {lp:.7f} criterion on log-probs {ref:.7f}")
    assert abs(lp - ref) < (1e-4 if precision == 0 else 2e-3), (lp, ref)
    if precision == 0:
        return
    # valid-position layout against the padded layout: the bars of test_valid_position_decoder_equals_padded_layout
    bc = dict(b, cap_len=_cap_len(b["masks"]))
    assert int(bc["cap_len"].sum()) < b["seqs"].size(0) * (b["seqs"].size(1) - 1)
    lc, gc = step(bc)
    rel = ((gc - gp).norm() / gp.norm()).item()
    print(f"valid positions: loss {lc:.7f} padded {lp:.7f} gradient rel {rel:.3e}")
    assert abs(lc - lp) < 2e-5 * max(1.0, abs(lp)), (lc, lp)
    assert rel < 2e-3, rel
    for e in m._entries:
        if e["kind"] == 2:
            continue
        sl = slice(e["offset"], e["offset"] + e["numel"])
        assert (gc[sl] - gp[sl]).norm().item() <= 2e-2 * gp[sl].norm().item() + 1e-6 * e["numel"] ** 0.5, e["name"]
