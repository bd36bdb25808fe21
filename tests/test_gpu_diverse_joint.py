"""The joint diverse executor (`executor="unfused_joint"`, ORTK_DEC_GROUPS_JOINT): the decoder passes of all groups of a global step
in one launch sequence, the selections of the step in one launch.
  * fp32 parity mode against the repaired reference's groups (golden G16, all six cases) with the assertions and bars of
    tests/test_gpu_diverse_beam.py::test_diverse_decode_vs_reference_golden;
  * the edge schedules of tests/diverse_joint_cases.py (one beam per group, two groups, more groups than positions, constraint and
    length penalty) against the CPU restatement with the same assertions, and against the staggered executor;
  * the exact properties in both precisions: two runs give the same bytes, lambda 0 makes every group group 0 (the joint pass runs
    all G blocks in every global step, so a row's bits do not depend on the step that computes it), the decoding constraint holds,
    the penalty moves something, group 0 is the plain search of the group's width;
  * mixed precision against the restatement under the oracle's teacher forcing, and with a sparse plan."""
import numpy as np
import pytest
import torch

import common as C
import diverse_beam_ref as D
import diverse_joint_cases as J
import helpers as H
from oracle import ort_oracle as O

pytestmark = pytest.mark.gpu

JOINT = "unfused_joint"


@pytest.fixture(scope="module")
def P():
    import sparse_image_captioning_amd as pkg
    pkg._lib.require_gpu()
    return pkg


def _model(P, cfg, state, precision=0):
    from sparse_image_captioning_amd.utils.config import Config
    m = P.get_model("relation_transformer")(Config(**cfg), precision=precision)
    missing, unexpected = m.load_state_dict(state, strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing), (missing, unexpected)
    return m.cuda().eval()


def _cuda(b):
    return {k: v.cuda() for k, v in b.items()}


def _decode(m, bt, opt):
    seq, lp = m(att_feats=bt["att_feats"], boxes=bt["boxes"], att_masks=bt["att_masks"], opt=opt, mode="sample")
    return seq.clone(), lp.clone(), m._last_decode[2].clone()


def close(a, b, tol):
    a = a.detach().float().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    np.testing.assert_allclose(a, b, rtol=tol, atol=tol)


@pytest.fixture(scope="module")
def tiny(P):
    return _model(P, C.TINY_CFG, H.g1_state())


def _against(m, seq, lp, b, G, cmp_, want_seq, want_lp, want_p, tag):
    """the assertions of test_diverse_decode_vs_reference_golden: images with a margin (cmp_) token-exact, log-probs and scores
    within 2e-4; every image: distinct captions and non-increasing scores per group, `model.beams` group by group"""
    bd = b // G
    n_img = seq.size(0)
    p = torch.tensor([[d["p"] for d in img] for img in m.beams])
    seq, lp = seq.cpu(), lp.cpu()
    assert seq.shape == (n_img, b, C.TINY_CFG["max_seq_length"]) and p.shape == (n_img, b)
    np.testing.assert_array_equal(seq.numpy()[cmp_], want_seq[cmp_], err_msg=tag)
    close(lp[torch.from_numpy(cmp_)], want_lp[cmp_], 2e-4)
    close(p[torch.from_numpy(cmp_)], want_p[cmp_], 2e-4)
    for n in range(n_img):
        for k in range(G):
            rows = slice(k * bd, (k + 1) * bd)
            assert len({tuple(r) for r in seq[n, rows].tolist()}) == bd, (tag, n, k)
            assert bool((p[n, rows][1:] <= p[n, rows][:-1]).all()), (tag, n, k, p[n].tolist())
        for k in range(b):
            ln = int((seq[n, k] != 0).sum())
            assert torch.equal(m.beams[n][k]["seq"].cpu(), seq[n, k, :ln]) and torch.equal(m.beams[n][k]["logps"].cpu(), lp[n, k, :ln])


@pytest.mark.parametrize("case", list(D.CASES))
def test_joint_decode_vs_reference_golden(P, golden, tiny, case):
    g = golden("g16_diverse_beam")
    b, G, opts, _, need = D.CASES[case]
    cmp_ = g[f"{case}/min_gap"] >= D.GAP
    assert int(cmp_.sum()) >= need
    bt = _cuda(H.torch_batch(D.case_inputs(C, int(g[f"{case}/seed"]))))
    seq, lp, _ = _decode(tiny, bt, dict(opts, beam_size=b, group_size=G, executor=JOINT))
    _against(tiny, seq, lp, b, G, cmp_, g[f"{case}/seq"], g[f"{case}/logprobs"], g[f"{case}/p"], case)


@pytest.mark.parametrize("case", list(J.EDGE_CASES))
def test_joint_edge_schedules_vs_restatement_and_staggered(P, tiny, case):
    """The window of active groups at its edges, against tests/diverse_beam_ref.py on the oracle; then the staggered executor on the
    same inputs: equal tokens on the images with a margin (whether all bytes are equal is printed, not asserted: the two executors
    run their GEMMs at different row counts)."""
    b, G, opts, seed, need = J.EDGE_CASES[case]
    cb, (oseq, olp, op_, gap) = J.restated(case)
    cmp_ = (gap >= D.GAP).numpy()
    assert int(cmp_.sum()) >= need and need * 2 >= D.N_IMG, (case, gap.tolist())
    bt = _cuda(cb)
    seq, lp, sc = _decode(tiny, bt, dict(opts, beam_size=b, group_size=G, executor=JOINT))
    _against(tiny, seq, lp, b, G, cmp_, oseq.numpy(), olp.numpy(), op_.numpy(), case)
    sseq, slp, ssc = _decode(tiny, bt, dict(opts, beam_size=b, group_size=G, executor="unfused"))
    same = torch.equal(seq, sseq) and torch.equal(lp, slp) and torch.equal(sc, ssc)
    print(f"[joint vs staggered, fp32] {case}: byte-equal outputs: {same}; images with a margin {int(cmp_.sum())} of {D.N_IMG}")
    np.testing.assert_array_equal(seq.cpu().numpy()[cmp_], sseq.cpu().numpy()[cmp_], err_msg=f"joint and staggered tokens differ: {case}")


@pytest.fixture(scope="module")
def margin_state2():
    """two full-width layers with real decision margins and no EOS bias (tests/test_gpu_diverse_beam.py::margin_state2)"""
    return H.torch_state(H.dense_param_shapes(dict(C.FULL_CFG, num_layers=2)), C.G2_SEED, C.G1_GEN_SCALE, 0.0)


@pytest.fixture(scope="module")
def wide_bf16(P, margin_state2):
    return _model(P, dict(C.FULL_CFG, num_layers=2), margin_state2, precision=1)


@pytest.fixture(scope="module")
def wide_batch():
    return H.torch_batch(C.make_inputs(seed=1716, n_img=6, n_reg=36, feat=2048, vocab=10001, spi=1, ragged=True))


# the property cases of tests/test_gpu_diverse_beam.py
PROPERTY_CASES = ((6, 3, {}), (4, 4, {}), (8, 2, {"decoding_constraint": 1, "length_penalty": "wu_0.7"}), (10, 5, {"diversity_lambda": 0.8}))


def _check_properties(m, bt, margin_of):
    """margin_of(b, G, opts) -> boolean mask of the images on which group 0 must equal the plain search token for token (fp32 parity
    mode: the images with a decision margin), or None: the share of equal images is printed (mixed precision: the joint pass and the
    plain search run their GEMMs at different row counts, so possibly in different kernels)."""
    pad = 0
    for b, G, opts in PROPERTY_CASES:
        bd = b // G
        opt = dict(opts, beam_size=b, group_size=G, executor=JOINT)
        first = _decode(m, bt, opt)
        again = _decode(m, bt, opt)
        for name, a, c in zip(("seq", "logprobs", "score"), first, again):
            assert torch.equal(a, c), ("two runs differ", name, b, G)
        assert bool((first[0][:, :, 0] != pad).all()), ("a row without a caption", b, G)
        # lambda 0: every group is group 0, bit for bit
        zero = _decode(m, bt, dict(opt, diversity_lambda=0.0))
        for k in range(1, G):
            for name, z in zip(("seq", "logprobs", "score"), zero):
                assert torch.equal(z[:, k * bd:(k + 1) * bd], z[:, :bd]), ("lambda 0: group differs from group 0", name, k, b, G)
        assert not torch.equal(first[0][:, bd:2 * bd], first[0][:, :bd]), ("the penalty moved nothing", b, G)
        # group 0 never sees a penalty: the plain search of width bd on the unfused executor (bd = 1: the greedy decode's tokens)
        plain_opt = {k: v for k, v in opts.items() if k != "diversity_lambda"}
        plain = _decode(m, bt, dict(plain_opt, beam_size=bd, executor="unfused"))
        eq = (first[0][:, :bd] == plain[0]).flatten(1).all(1).cpu()
        mask = margin_of(b, G, opts)
        if mask is None:
            print(f"[joint, mixed precision] b={b} G={G}: group 0 equals the plain width-{bd} search on {eq.float().mean().item():.3f} of the images")
        else:
            assert bool(eq[mask].all()), ("group 0 is not the plain beam search", b, G, eq.tolist(), mask.tolist())
        if opts.get("decoding_constraint"):
            seq = first[0]
            rep = (seq[..., 1:] == seq[..., :-1]) & (seq[..., 1:] != pad)
            assert not bool(rep.any()), ("a token repeats its predecessor", b, G)


def test_joint_exact_properties_fp32(P, tiny):
    cb = H.g1_batch()
    state, cfg = H.g1_state(), J.oracle_cfg()

    def margin_of(b, G, opts):
        with torch.no_grad():
            gap = D.diverse_beam_search(state, cfg, cb["att_feats"], cb["boxes"], cb["att_masks"], b, G, **opts)[3]
        return gap >= D.GAP

    _check_properties(tiny, _cuda(cb), margin_of)


def test_joint_exact_properties_bf16(P, wide_bf16, wide_batch):
    """... in mixed precision on full-width layers and the 10 001-token vocabulary (the generator's block statistics, the fast
    exponential, bf16 caches through the row kernel's lk_row instance)"""
    _check_properties(wide_bf16, _cuda(wide_batch), lambda b, G, opts: None)


def test_joint_exact_properties_with_a_sparse_plan(P):
    """The case of test_exact_properties_with_a_sparse_plan on the joint executor: two runs, lambda 0, a caption in every row; group 0
    against the plain search is printed (mixed precision)."""
    cfg = dict(C.FULL_CFG, num_layers=2)
    dense = H.torch_state(H.dense_param_shapes(cfg), C.G2_SEED, C.G1_GEN_SCALE, 0.0)
    g = torch.Generator().manual_seed(23)
    state = {k: (v * (torch.rand(v.shape, generator=g) < 0.05).float() if v.dim() >= 2 and "generator" not in k and "embed" not in k else v)
             for k, v in dense.items()}
    m = _model(P, cfg, state, precision=1)
    m.enable_sparse_kernels()
    bt = _cuda(H.torch_batch(C.make_inputs(seed=1717, n_img=4, n_reg=36, feat=2048, vocab=10001, spi=1, ragged=True)))
    opt = {"beam_size": 6, "group_size": 3, "executor": JOINT}
    first = _decode(m, bt, opt)
    again = _decode(m, bt, opt)
    plain = _decode(m, bt, {"beam_size": 2, "executor": "unfused"})
    zero = _decode(m, bt, dict(opt, diversity_lambda=0.0))
    for name, a, c, z in zip(("seq", "logprobs", "score"), first, again, zero):
        assert torch.equal(a, c), name
        for k in range(1, 3):
            assert torch.equal(z[:, 2 * k:2 * k + 2], z[:, :2]), (name, k)
    assert bool((first[0][:, :, 0] != 0).all())
    eq = (first[0][:, :2] == plain[0]).flatten(1).all(1).float().mean().item()
    print(f"[joint, sparse plan] group 0 equals the plain width-2 search on {eq:.3f} of the images")


@pytest.mark.parametrize("b,G,lam", [(6, 3, 0.5), (32, 4, 0.3)])
def test_joint_bf16_decode_vs_restatement(P, margin_state2, wide_bf16, wide_batch, b, G, lam):
    """As test_bf16_diverse_decode_vs_restatement: EVERY returned row reproduces under the oracle's teacher forcing within 0.05,
    position by position; the share of rows equal to the restatement's is printed."""
    cfg = J.oracle_cfg(dict(C.FULL_CFG, num_layers=2))
    cb = wide_batch
    with torch.no_grad():
        oseq, _, _, _ = D.diverse_beam_search(margin_state2, cfg, cb["att_feats"], cb["boxes"], cb["att_masks"], b, G, diversity_lambda=lam)
    seq, lp, _ = _decode(wide_bf16, _cuda(cb), {"beam_size": b, "group_size": G, "diversity_lambda": lam, "executor": JOINT})
    seq, lp = seq.cpu(), lp.cpu()
    idx = torch.arange(seq.size(0)).repeat_interleave(b)
    sub = {k: cb[k][idx] for k in ("att_feats", "boxes", "att_masks")}
    rows = seq.view(-1, seq.size(-1))
    tf_in = torch.cat([rows.new_full((rows.size(0), 1), C.BOS), rows], 1)
    with torch.no_grad():
        tf_lp = O.forward_logp(margin_state2, cfg, sub["att_feats"], sub["boxes"], tf_in, sub["att_masks"], rollouts=True)
    tf_lp = tf_lp.gather(2, rows.unsqueeze(2)).squeeze(2)
    dev_ = ((tf_lp - lp.view_as(tf_lp)) * (rows != 0)).abs().max(1).values
    row_eq = (seq == oseq).all(-1)
    print(f"[joint bf16 vs restatement] b={b} G={G} lambda={lam}: {row_eq.float().mean().item():.3f} of the rows equal "
          f"(group 0 alone {row_eq[:, :b // G].float().mean().item():.3f}); teacher-forced log-probs of all {rows.size(0)} rows: worst {dev_.max().item():.4f}")
    assert dev_.max().item() < 0.05, dev_.max().item()
    assert bool((seq[:, :, 0] != 0).all())
