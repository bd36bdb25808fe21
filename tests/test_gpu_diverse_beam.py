"""Diverse beam search on the device (ortk_decode_opts.group_size > 1; the grouped selection step beam_step_diverse_kernel):
  * the operator entry ortk_beam_select_diverse — the device function of the grouped step — against numpy's float64 lexsort on
    operands for which every fp32 operation is exact (ties included), fused against the float64 log-soft-max where the decisive
    gap is wide enough, and without penalty entries against ortk_beam_select byte for byte;
  * the decode against the repaired reference's groups (golden G16), its exact properties (group 0 is the plain beam search of
    the group's width, lambda 0 makes every group that search, two runs give the same bytes, the decoding constraint holds in
    every group) in both precisions on every executor that serves it, mixed precision against the CPU restatement, the limits, and
    SCST with grouped beam-search rollouts."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import common as C
import diverse_beam_ref as D
import helpers as H
from oracle import ort_oracle as O

pytestmark = pytest.mark.gpu

EXECUTORS = ("unfused", "auto")           # the executors that serve group_size > 1 ("auto" resolves to the unfused one)


@pytest.fixture(scope="module")
def P():
    import sparse_image_captioning_amd as pkg
    pkg._lib.require_gpu()
    return pkg


def _model(P, cfg, state, precision=0, **over):
    from sparse_image_captioning_amd.utils.config import Config
    m = P.get_model("relation_transformer")(Config(**dict(cfg, **over)), precision=precision)
    missing, unexpected = m.load_state_dict(state, strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing), (missing, unexpected)
    return m.cuda().eval()


def _cuda(b):
    return {k: v.cuda() for k, v in b.items()}


def _oracle_cfg(cfg):
    return O.OCfg(**{k: v for k, v in cfg.items() if not k.startswith("prune")})


def close(a, b, tol):
    a = a.detach().float().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    np.testing.assert_allclose(a, b, rtol=tol, atol=tol)


# ------------------------------------------------------------------------------------------------ operator
N_IMG = 3
WIDTHS = (1, 2, 5, 8, 9, 16)
VOCABS = (33, 257, 10001, 10240)
LAMBDA = 0.5
# log-probs and cumulative scores on a dyadic grid (multiples of 2^-6, magnitude below 64) and lambda 0.5 with counts <= 31: every
# difference and sum below is a multiple of 2^-6 of magnitude below 144 — 14 significant bits, exact in fp32 — so numpy's float64
# arithmetic and lexsort are the reference WITH ties
LEVELS = np.array([-48.0, -6.0, -4.5, -3.015625, -3.0, -2.0, -1.5, -1.0, -0.515625, -0.5], np.float32)
LEVEL_P = (0.9, 0.04, 0.03, 0.01, 0.008, 0.005, 0.003, 0.002, 0.001, 0.001)       # a thin top: ties at the cut, not only far above it
CUM_LEVELS = np.array([-63.984375, -3.0, -2.5, -1.0, 0.0], np.float32)


def _padded(x, ld):
    """(rows, V) -> device (rows, ld) with NaN in the pad columns (never read)"""
    out = np.full((x.shape[0], ld), np.nan, np.float32)
    out[:, :x.shape[1]] = x
    return torch.from_numpy(out).cuda()


def _select_diverse(L, zd, ld, cum, prev, pen, n_pen, lam, n_img, q, b, V, fused, scale):
    val = torch.empty(n_img, b, device="cuda")
    par = torch.empty(n_img, b, dtype=torch.int32, device="cuda")
    tok = torch.empty(n_img, b, dtype=torch.int32, device="cuda")
    tlp = torch.empty(n_img, b, device="cuda")
    rc = L.lib().ortk_beam_select_diverse(L.ptr(zd), ld, L.ptr(cum), L.ptr(prev) if prev is not None else None,
                                          L.ptr(pen) if pen is not None else None, n_pen, lam, n_img, q, b, V, fused, scale,
                                          L.ptr(val), L.ptr(par), L.ptr(tok), L.ptr(tlp), L.stream_ptr())
    assert rc == 0, rc
    return val, par, tok, tlp


def _select_plain(L, zd, ld, cum, prev, n_img, q, b, V, fused, scale):
    val = torch.empty(n_img, b, device="cuda")
    par = torch.empty(n_img, b, dtype=torch.int32, device="cuda")
    tok = torch.empty(n_img, b, dtype=torch.int32, device="cuda")
    rc = L.lib().ortk_beam_select(L.ptr(zd), ld, L.ptr(cum), L.ptr(prev) if prev is not None else None, n_img, q, b, V, fused, scale,
                                  L.ptr(val), L.ptr(par), L.ptr(tok), L.stream_ptr())
    assert rc == 0, rc
    return val, par, tok


def _counts(pen, n_img, V):
    """(n_img, V) float64: how often every token is listed (-1 and tokens outside the vocabulary: never)"""
    cnt = np.zeros((n_img, V))
    for i in range(n_img):
        for v in pen[i]:
            if 0 <= v < V:
                cnt[i, v] += 1
    return cnt


def _expected(logp, cum, cnt, lam, prev, n_img, q, b, V):
    """float64: the b best of every image's (q, V) values cum + (logp - cnt * lam) by (larger value, lower flat index), the previous
    tokens left out -> val, parent, token, the picks' unaugmented logp, and the gap between ranks b and b + 1 and inside the top b"""
    ev, ep, et, el, gaps = [], [], [], [], []
    for i in range(n_img):
        lp = logp[i * q:(i + 1) * q].astype(np.float64)
        v = cum[i * q:(i + 1) * q].astype(np.float64)[:, None] + (lp - cnt[i][None, :] * lam)
        ok = np.ones((q, V), bool)
        if prev is not None:
            ok[np.arange(q), prev[i * q:(i + 1) * q]] = False
        flat = np.flatnonzero(ok.ravel())
        vv = v.ravel()[flat]
        order = np.lexsort((flat, -vv))[:b + 1]
        win = flat[order[:b]]
        top = vv[order]
        gaps.append(np.min(top[:-1] - top[1:]) if top.size > 1 else np.inf)
        ev.append(v.ravel()[win]); ep.append(win // V); et.append(win % V); el.append(lp.ravel()[win])
    return np.stack(ev), np.stack(ep).astype(np.int32), np.stack(et).astype(np.int32), np.stack(el), np.array(gaps)


def _pen_list(rs, n_pen, z, cum, prev, q, b, V):
    """(N_IMG, n_pen) int32 with: the unpenalised winners' tokens (so the penalty changes the pick), repeated tokens, a token that is
    also a row's `prev`, and -1 entries"""
    pen = rs.randint(0, V, size=(N_IMG, max(n_pen, 1))).astype(np.int32)[:, :n_pen]
    if n_pen == 0:
        return pen
    _, _, wtok, _, _ = _expected(z, cum, np.zeros((N_IMG, V)), 0.0, prev, N_IMG, q, b, V)
    for i in range(N_IMG):
        k = min(n_pen, b)
        pen[i, :k] = wtok[i, :k]                                   # the winners
        if n_pen >= 3:
            pen[i, 2] = pen[i, 0]                                  # a repeated token (count 2)
        if n_pen >= 6:
            pen[i, 3] = pen[i, 4] = pen[i, 5] = pen[i, 1]          # ... and one with count 4
        if prev is not None and n_pen >= 2:
            pen[i, n_pen - 1] = prev[i * q]                        # a penalised token that no row 0 candidate can be anyway
        if n_pen >= 8:
            pen[i, 6] = -1                                         # holes
            pen[i, n_pen - 2] = -1
    return pen


@pytest.mark.parametrize("V", VOCABS)
def test_operator_exact_order_with_ties(P, V):
    """fused = 0, operands on the dyadic grid: val, parent, token equal float64 numpy's lexsort by (-value, flat index), tok_lp the
    unaugmented entry, a second run returns the same bytes, and without penalty entries the result is ortk_beam_select's."""
    L = P._lib
    ld = (V + 127) // 128 * 128
    rs = np.random.RandomState(6000 + V)
    case = moved = with_pen = 0
    for b in WIDTHS:
        for q in sorted({1, b}):
            for n_pen in sorted({0, 1, b, 31}):
                rows = N_IMG * q
                z = LEVELS[rs.choice(len(LEVELS), size=(rows, V), p=LEVEL_P)]
                cum = CUM_LEVELS[rs.randint(0, len(CUM_LEVELS), size=rows)].copy()
                prev = None
                if case % 2:
                    prev = rs.randint(0, V, size=rows).astype(np.int32)
                    prev[0::3] = z[0::3].argmax(1)                        # ... the row's best entry among them
                case += 1
                pen = _pen_list(rs, n_pen, z, cum, prev, q, b, V)
                cnt = _counts(pen, N_IMG, V)
                wv, wp, wt, wl, _ = _expected(z, cum, cnt, LAMBDA, prev, N_IMG, q, b, V)
                assert np.array_equal(wv.astype(np.float32).astype(np.float64), wv)        # (exact in fp32, as claimed above)
                zd, cd = _padded(z, ld), torch.from_numpy(cum).cuda()
                pd = None if prev is None else torch.from_numpy(prev).cuda()
                pend = torch.from_numpy(np.ascontiguousarray(pen)).cuda() if n_pen else None
                runs = [[o.cpu().numpy() for o in _select_diverse(L, zd, ld, cd, pd, pend, n_pen, LAMBDA, N_IMG, q, b, V, 0, 1.0)] for _ in range(2)]
                for a, c in zip(*runs):
                    assert a.tobytes() == c.tobytes(), ("two runs differ", V, b, q, n_pen)
                tag = f"V={V} b={b} q={q} n_pen={n_pen} prev={prev is not None}"
                for name, got, w in zip(("val", "parent", "token", "tok_lp"), runs[0], (wv.astype(np.float32), wp, wt, wl.astype(np.float32))):
                    np.testing.assert_array_equal(got, w, err_msg=f"{name} {tag}")
                if n_pen == 0:
                    plain = [o.cpu().numpy() for o in _select_plain(L, zd, ld, cd, pd, N_IMG, q, b, V, 0, 1.0)]
                    for a, c in zip(runs[0][:3], plain):
                        assert a.tobytes() == c.tobytes(), ("ortk_beam_select differs", tag)
                else:
                    _, up, ut, _, _ = _expected(z, cum, np.zeros((N_IMG, V)), 0.0, prev, N_IMG, q, b, V)
                    with_pen += 1
                    moved += int(not (np.array_equal(up, wp) and np.array_equal(ut, wt)))
    assert moved >= with_pen * 3 // 4, (moved, with_pen)          # the penalty changed the pick


F_IMG = 8


@pytest.mark.parametrize("V", VOCABS)
def test_operator_fused_vs_float64_log_softmax(P, V):
    """fused = 1 (raw logits, exact expf, scale 1 and 1 / 0.7) against float64: images whose closest pair among the best b + 1
    candidates lies at least GAP apart pick the float64 order's parents and tokens; val and tok_lp within 2e-5 — |logit * scale| < 32
    (half an ulp 1.9e-6) in the term, as much in the maximum and the log-sum-exp, 1.9e-6 in the sum with |cum| < 64 and the
    penalty's subtraction, doubled.  At most a quarter of the images fall below GAP (normal logits of deviation 3: the best 17 of up
    to 164 000 candidates lie ~0.02 apart)."""
    L = P._lib
    ld = (V + 127) // 128 * 128
    rs = np.random.RandomState(7000 + V)
    total = left_out = 0
    lam = float(np.float32(0.3))
    for b in (1, 5, 9, 16):
        for q in sorted({1, b}):
            for n_pen in (0, b, 31):
                rows = F_IMG * q
                z = (3.0 * rs.randn(rows, V)).astype(np.float32)
                cum = (-4.0 * rs.uniform(size=rows)).astype(np.float32)
                prev = rs.randint(0, V, size=rows).astype(np.int32)
                pen = rs.randint(0, V, size=(F_IMG, max(n_pen, 1))).astype(np.int32)[:, :n_pen]
                for i in range(F_IMG):
                    best = np.argsort(-z[i * q])[:n_pen]                 # the best tokens of the image's first row, some twice
                    pen[i, :best.size] = best
                    if n_pen >= 4:
                        pen[i, 3] = pen[i, 0]
                cnt = _counts(pen, F_IMG, V)
                zd, cd, pd = _padded(z, ld), torch.from_numpy(cum).cuda(), torch.from_numpy(prev).cuda()
                pend = torch.from_numpy(np.ascontiguousarray(pen)).cuda() if n_pen else None
                for scale in (1.0, 1.0 / 0.7):
                    x = z.astype(np.float64) * float(np.float32(scale))
                    mx = x.max(1, keepdims=True)
                    lsm = x - mx - np.log(np.exp(x - mx).sum(1, keepdims=True))
                    wv, wp, wt, wl, gaps = _expected(lsm, cum, cnt, lam, prev, F_IMG, q, b, V)
                    val, par, tok, tlp = [o.cpu().numpy() for o in _select_diverse(L, zd, ld, cd, pd, pend, n_pen, lam, F_IMG, q, b, V, 1, float(np.float32(scale)))]
                    ok = gaps >= D.GAP
                    total += F_IMG
                    left_out += int((~ok).sum())
                    tag = f"V={V} b={b} q={q} n_pen={n_pen} scale={scale}"
                    np.testing.assert_array_equal(par[ok], wp[ok], err_msg="parent " + tag)
                    np.testing.assert_array_equal(tok[ok], wt[ok], err_msg="token " + tag)
                    np.testing.assert_allclose(val[ok], wv[ok], rtol=0, atol=2e-5, err_msg="val " + tag)
                    np.testing.assert_allclose(tlp[ok], wl[ok], rtol=0, atol=2e-5, err_msg="tok_lp " + tag)
                    if n_pen == 0:
                        plain = [o.cpu().numpy() for o in _select_plain(L, zd, ld, cd, pd, F_IMG, q, b, V, 1, float(np.float32(scale)))]
                        for a, c in zip((val, par, tok), plain):
                            assert a.tobytes() == c.tobytes(), ("ortk_beam_select differs", tag)
    print(f"[diverse operator, fused] V={V}: {left_out} of {total} images below GAP")
    assert left_out * 4 <= total, (left_out, total)


def test_operator_refuses_bad_arguments(P):
    L = P._lib
    V, b = 33, 4
    z = torch.zeros(b, 128, device="cuda")
    cum = torch.zeros(b, device="cuda")
    pen = torch.zeros(1, 32, dtype=torch.int32, device="cuda")
    out = (torch.empty(1, b, device="cuda"), torch.empty(1, b, dtype=torch.int32, device="cuda"), torch.empty(1, b, dtype=torch.int32, device="cuda"),
           torch.empty(1, b, device="cuda"))

    def rc(n_pen=2, lam=0.5, q=b, bb=b, pen_=pen):
        return L.lib().ortk_beam_select_diverse(L.ptr(z), 128, L.ptr(cum), None, L.ptr(pen_) if pen_ is not None else None, n_pen, lam, 1, q, bb, V, 0,
                                                1.0, *(L.ptr(o) for o in out), L.stream_ptr())

    assert rc() == 0 and rc(n_pen=31) == 0 and rc(n_pen=0, pen_=None) == 0 and rc(lam=0.0) == 0
    for kw in ({"n_pen": -1}, {"n_pen": 32}, {"lam": -0.5}, {"lam": float("nan")}, {"lam": float("inf")}, {"q": 2}, {"bb": 33}, {"n_pen": 2, "pen_": None}):
        assert rc(**kw) == -1, kw
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ decode
def _decode(m, bt, opt):
    seq, lp = m(att_feats=bt["att_feats"], boxes=bt["boxes"], att_masks=bt["att_masks"], opt=opt, mode="sample")
    return seq, lp, m._last_decode[2]


@pytest.fixture(scope="module")
def tiny(P):
    return _model(P, C.TINY_CFG, H.g1_state())


@pytest.mark.parametrize("executor", EXECUTORS)
@pytest.mark.parametrize("case", list(D.CASES))
def test_diverse_decode_vs_reference_golden(P, golden, tiny, case, executor):
    """Fp32 parity mode against the repaired reference's groups (golden G16).  Images whose closest decision of the whole search is
    at least GAP wide: tokens exact, log-probs and scores within 2e-4.  Every image: the captions of a group are distinct and its
    scores non-increasing; `model.beams` lists them group by group."""
    g = golden("g16_diverse_beam")
    b, G, opts, _, need = D.CASES[case]
    bd = b // G
    cmp_ = g[f"{case}/min_gap"] >= D.GAP
    assert int(cmp_.sum()) >= need
    bt = _cuda(H.torch_batch(D.case_inputs(C, int(g[f"{case}/seed"]))))
    seq, lp, _ = _decode(tiny, bt, dict(opts, beam_size=b, group_size=G, executor=executor))
    p = torch.tensor([[d["p"] for d in img] for img in tiny.beams])
    seq, lp = seq.cpu(), lp.cpu()
    assert seq.shape == (D.N_IMG, b, C.TINY_CFG["max_seq_length"]) and p.shape == (D.N_IMG, b)
    np.testing.assert_array_equal(seq.numpy()[cmp_], g[f"{case}/seq"][cmp_])
    close(lp[torch.from_numpy(cmp_)], g[f"{case}/logprobs"][cmp_], 2e-4)
    close(p[torch.from_numpy(cmp_)], g[f"{case}/p"][cmp_], 2e-4)
    for n in range(D.N_IMG):
        for k in range(G):
            rows = slice(k * bd, (k + 1) * bd)
            assert len({tuple(r) for r in seq[n, rows].tolist()}) == bd, (case, n, k)
            assert bool((p[n, rows][1:] <= p[n, rows][:-1]).all()), (case, n, k, p[n].tolist())
        for k in range(b):
            ln = int((seq[n, k] != 0).sum())                            # (as `beams` cuts a row)
            assert torch.equal(tiny.beams[n][k]["seq"].cpu(), seq[n, k, :ln]) and torch.equal(tiny.beams[n][k]["logps"].cpu(), lp[n, k, :ln])


@pytest.fixture(scope="module")
def margin_state2():
    """Two full-width layers with real decision margins (generator x 3 as tests/test_gpu_model.py::margin_state) and NO EOS bias:
    with two layers that bias ends every caption after one or two tokens; without it the groups run 1 .. 18 positions."""
    return H.torch_state(H.dense_param_shapes(dict(C.FULL_CFG, num_layers=2)), C.G2_SEED, C.G1_GEN_SCALE, 0.0)


@pytest.fixture(scope="module")
def wide_bf16(P, margin_state2):
    return _model(P, dict(C.FULL_CFG, num_layers=2), margin_state2, precision=1)


@pytest.fixture(scope="module")
def wide_batch():
    return H.torch_batch(C.make_inputs(seed=1716, n_img=6, n_reg=36, feat=2048, vocab=10001, spi=1, ragged=True))


PROPERTY_CASES = ((6, 3, {}), (4, 4, {}), (8, 2, {"decoding_constraint": 1, "length_penalty": "wu_0.7"}), (10, 5, {"diversity_lambda": 0.8}))


def _check_properties(m, bt, executor):
    pad = 0
    for b, G, opts in PROPERTY_CASES:
        bd = b // G
        opt = dict(opts, beam_size=b, group_size=G, executor=executor)
        first = [x.clone() for x in _decode(m, bt, opt)]
        again = _decode(m, bt, opt)
        for name, a, c in zip(("seq", "logprobs", "score"), first, again):
            assert torch.equal(a, c), ("two runs differ", name, b, G, executor)
        plain_opt = {k: v for k, v in opts.items() if k != "diversity_lambda"}
        # group 0 never sees a penalty: the plain beam search of width bd on the same executor — the unfused one, which "auto" resolves
        # to for group_size > 1 — bit for bit (bd = 1: the greedy decode's tokens)
        plain = _decode(m, bt, dict(plain_opt, beam_size=bd, executor="unfused"))
        if bd > 1:
            for name, a, c in zip(("seq", "logprobs", "score"), first, plain):
                assert torch.equal(a[:, :bd], c), ("group 0 is not the plain beam search", name, b, G, executor)
        else:
            assert torch.equal(first[0][:, :1], plain[0]), ("group 0 is not the greedy decode", b, G, executor)
        assert not torch.equal(first[0][:, bd:2 * bd], first[0][:, :bd]), ("the penalty moved nothing", b, G, executor)
        # lambda 0: every group is group 0
        zero = _decode(m, bt, dict(opt, diversity_lambda=0.0))
        for k in range(G):
            for name, a, c in zip(("seq", "logprobs", "score"), zero, first):
                assert torch.equal(a[:, k * bd:(k + 1) * bd], c[:, :bd]), ("lambda 0: group differs from group 0", name, k, b, G, executor)
        if opts.get("decoding_constraint"):
            seq = first[0]
            rep = (seq[..., 1:] == seq[..., :-1]) & (seq[..., 1:] != pad)
            assert not bool(rep.any()), ("a token repeats its predecessor", b, G, executor)


@pytest.mark.parametrize("executor", EXECUTORS)
def test_exact_properties_fp32(P, tiny, executor):
    _check_properties(tiny, _cuda(H.g1_batch()), executor)


@pytest.mark.parametrize("executor", EXECUTORS)
def test_exact_properties_bf16(P, wide_bf16, wide_batch, executor):
    """... in mixed precision on full-width layers and the 10 001-token vocabulary: the generator's block statistics and the fast
    exponential are those of the plain beam step."""
    _check_properties(wide_bf16, _cuda(wide_batch), executor)


def test_exact_properties_with_a_sparse_plan(P):
    """A per-linear sparse plan (enable_sparse_kernels on zero-filled weights) serves group_size > 1 through the same driver."""
    cfg = dict(C.FULL_CFG, num_layers=2)
    dense = H.torch_state(H.dense_param_shapes(cfg), C.G2_SEED, C.G1_GEN_SCALE, 0.0)
    g = torch.Generator().manual_seed(23)
    state = {k: (v * (torch.rand(v.shape, generator=g) < 0.05).float() if v.dim() >= 2 and "generator" not in k and "embed" not in k else v)
             for k, v in dense.items()}
    m = _model(P, cfg, state, precision=1)
    m.enable_sparse_kernels()
    bt = _cuda(H.torch_batch(C.make_inputs(seed=1717, n_img=4, n_reg=36, feat=2048, vocab=10001, spi=1, ragged=True)))
    opt = {"beam_size": 6, "group_size": 3, "executor": "unfused"}
    first = [x.clone() for x in _decode(m, bt, opt)]
    again = _decode(m, bt, opt)
    plain = _decode(m, bt, {"beam_size": 2, "executor": "unfused"})
    zero = _decode(m, bt, dict(opt, diversity_lambda=0.0))
    for name, a, c, p_, z in zip(("seq", "logprobs", "score"), first, again, plain, zero):
        assert torch.equal(a, c), name
        assert torch.equal(a[:, :2], p_), name
        for k in range(3):
            assert torch.equal(z[:, 2 * k:2 * k + 2], p_), (name, k)


def _tf_logp_oracle(Pm, cfg, cb, rows):
    tf_in = torch.cat([rows.new_full((rows.size(0), 1), C.BOS), rows], 1)
    with torch.no_grad():
        return O.forward_logp(Pm, cfg, cb["att_feats"], cb["boxes"], tf_in, cb["att_masks"], rollouts=True)


@pytest.mark.parametrize("b,G,lam", [(6, 3, 0.5), (32, 4, 0.3)])
def test_bf16_diverse_decode_vs_restatement(P, margin_state2, wide_bf16, wide_batch, b, G, lam):
    """Mixed precision against tests/diverse_beam_ref.py on weights with real margins.  EVERY returned row is a real, correctly
    scored hypothesis: the oracle's teacher-forced log-probs of its tokens lie within 0.05 of the (unaugmented) log-probs the decode
    returned, position by position (the bar of tests/test_gpu_beam_wide.py for the same check).  The share of rows equal to the
    restatement's row of the same group and rank is printed, not asserted: bf16 activations cannot order close ranks, and a
    different pick in one group moves the penalties of every later group (measured: profiles/diverse_beam.txt)."""
    cfg = _oracle_cfg(dict(C.FULL_CFG, num_layers=2))
    cb = wide_batch
    with torch.no_grad():
        oseq, olp, _, _ = D.diverse_beam_search(margin_state2, cfg, cb["att_feats"], cb["boxes"], cb["att_masks"], b, G, diversity_lambda=lam)
    seq, lp, _ = _decode(wide_bf16, _cuda(cb), {"beam_size": b, "group_size": G, "diversity_lambda": lam, "executor": "unfused"})
    seq, lp = seq.cpu(), lp.cpu()
    n_img = seq.size(0)
    idx = torch.arange(n_img).repeat_interleave(b)
    sub = {k: cb[k][idx] for k in ("att_feats", "boxes", "att_masks")}
    rows = seq.view(-1, seq.size(-1))
    tf_lp = _tf_logp_oracle(margin_state2, cfg, sub, rows).gather(2, rows.unsqueeze(2)).squeeze(2)
    dev_ = ((tf_lp - lp.view_as(tf_lp)) * (rows != 0)).abs().max(1).values
    row_eq = (seq == oseq).all(-1)
    g0 = row_eq[:, :b // G].float().mean().item()
    print(f"[diverse bf16 vs restatement] b={b} G={G} lambda={lam}: {row_eq.float().mean().item():.3f} of the rows equal "
          f"(group 0 alone {g0:.3f}); teacher-forced log-probs of all {rows.size(0)} rows: worst {dev_.max().item():.4f}")
    assert dev_.max().item() < 0.05, dev_.max().item()
    assert bool((seq[:, :, 0] != 0).all())                              # every row holds a caption


def test_limits(P, tiny):
    """Refused combinations fail in Python before any device work; decode_supported, the workspace query and ortk_decode agree."""
    L = P._lib
    m, bt = tiny, _cuda(H.g1_batch())
    kw = dict(att_feats=bt["att_feats"], boxes=bt["boxes"], att_masks=bt["att_masks"], mode="sample")
    B, S = bt["att_feats"].shape[:2]
    T = C.TINY_CFG["max_seq_length"]
    for opt, why in (({"beam_size": 6, "group_size": 4}, "not a multiple"), ({"beam_size": 3, "group_size": 6}, "exceeds beam_size"),
                     ({"beam_size": 4, "group_size": 2, "diversity_lambda": -0.5}, "finite number >= 0"),
                     ({"beam_size": 0, "num_random_sample": 3, "group_size": 2}, "beam decodes"),
                     ({"beam_size": 4, "group_size": 2, "executor": "stack"}, "does not serve group_size")):
        with pytest.raises(ValueError, match=why):
            m(**kw, opt=opt)
        assert not m.decode_supported(B, S, opt), opt
    assert m.decode_supported(B, S, {"beam_size": 4, "group_size": 2})
    lib = L.lib()
    feats, bxs, masks = m._prepare(bt["att_feats"], bt["boxes"], bt["att_masks"])
    o, K, _ = m._decode_opts({"beam_size": 6, "group_size": 3, "seed": 0})
    good = lib.ortk_decode_workspace_bytes(Ct.byref(m._ccfg), B, S, Ct.byref(o))
    assert good > 0
    ws = torch.empty(int(good) * 2, dtype=torch.uint8, device="cuda")
    seq = torch.zeros(B, 6, T, dtype=torch.long, device="cuda")
    lp = torch.zeros(B, 6, T, device="cuda")
    sc = torch.zeros(B, 6, device="cuda")

    def run(oo, nbytes):
        return lib.ortk_decode(Ct.byref(m._ccfg), m._eff_params_ptr(False, 0), L.ptr(feats), L.ptr(bxs), L.ptr(masks), B, S, Ct.byref(oo), L.ptr(ws),
                               nbytes, L.ptr(seq), L.ptr(lp), L.ptr(sc), L.stream_ptr())

    assert run(o, int(good)) == 0
    assert run(o, int(good) - 256) == -2                                 # ORTK_ENOSPC: the query is what the decode carves
    want = _decode(m, bt, {"beam_size": 6, "group_size": 3})
    assert torch.equal(seq, want[0]) and torch.equal(sc, want[2])
    for field, value in (("group_size", 4), ("group_size", 12), ("group_size", -1), ("diversity_lambda", -0.25), ("diversity_lambda", float("nan")),
                         ("exec_flags", L.DEC_STACK), ("exec_flags", L.DEC_SPARSE_STREAM), ("num_random_sample", 2)):
        bad = L.DecodeOpts.from_buffer_copy(o)
        setattr(bad, field, value)
        assert lib.ortk_decode_workspace_bytes(Ct.byref(m._ccfg), B, S, Ct.byref(bad)) == 0, (field, value)
        assert run(bad, ws.numel()) == -1, (field, value)                # ORTK_EINVAL
    torch.cuda.synchronize()


def test_scst_grouped_beam_search_rollouts(P):
    """`scst_step(sample="beam_search", rollout_opt={"group_size": 2})`: the rollouts are the diverse decode of the same options."""
    from sparse_image_captioning_amd.training import NativeTrainer
    ns = 4
    cb = H.g1_batch()
    m, b = _model(P, C.TINY_CFG, H.g1_state()), _cuda(cb)
    N = cb["att_feats"].size(0)
    rw = torch.linspace(-1.0, 1.0, N * ns)
    want, _, _ = _decode(m, b, {"beam_size": ns, "group_size": 2})
    want = want.clone()
    plain, _, _ = _decode(m, b, {"beam_size": ns})
    assert not torch.equal(want, plain)
    tr = NativeTrainer(m, noamopt_factor=1.0, noamopt_warmup=10)
    m.train()
    loss, reward, seq, greedy = tr.scst_step(b, lambda s_, g_: rw, num_samples=ns, baseline="greedy", sample="beam_search",
                                             rollout_opt={"group_size": 2})
    assert torch.equal(seq, want)
    assert bool(torch.isfinite(loss).all())
