"""CPU checks of tests/chain_ref.py (read its docstring first), the yardstick of tests/test_gpu_row_chain.py:

  * an fp32 numpy restatement of every stage of the forward and the backward chain, in the kernel's order of arithmetic (32-input
    k-steps into one fp32 running sum; the LayerNorm's lane chains, shuffles and the tree over the eight column waves), stays within
    ONE bound of the float64 reference on every input class, and the bf16 outputs inside their intervals;
  * eight mutants of that restatement are caught by the bars (4 bounds / the bf16 interval) or by the bit checks of the routing
    operands -- MUTANTS states which check is expected to see each, test_mutant asserts it and prints the figures;
  * the restated launch geometry equals ortk_row_chain_plan / ortk_row_bchain_plan over the case table and a sweep of M, the plan
    refuses what the operator refuses, and the case table hits every geometry class.

The dropout draws are chain_ref.keep, the restatement of the kernels' hash (the GPU file asserts it equal to ortk_dropout_apply)."""
import ctypes as C

import numpy as np
import pytest

import chain_ref as CR
import ln_ref as R

F32 = np.float32
D, NC, FF = 512, 4, 2048
M_HOST = 40                      # 8 rows of each of the five input classes
SEEDS = dict(r=1111, h=2222, o=3333, a=4321, b=8765)
CLASS_SCALE = np.array([2.0, 2.0, 1e-3, 1e-6, 1e-3])


def _bf(x):
    return CR.bf16_rn(np.asarray(x, dtype=F32))


# ------------------------------------------------------------------------------------------------ the fp32 restatement
def mm32(a, w, skip_kstep=None):
    """a w^T as the kernels sum it: 32 inputs per k-step (one MFMA), the k-steps into one fp32 running sum."""
    a, w = np.asarray(a, dtype=F32), np.asarray(w, dtype=F32)
    acc = np.zeros((a.shape[0], w.shape[0]), dtype=F32)
    for ks in range(a.shape[1] // 32):
        if ks == skip_kstep:
            continue
        acc = (acc + a[:, 32 * ks:32 * ks + 32] @ w[:, 32 * ks:32 * ks + 32].T).astype(F32)
    return acc


def _lanes(x):
    """(rows, 512) -> (rows, wave 8, q 4, 16 values of a lane in the order the kernel adds them): column = 64 w + 16 nt + 4 q + r."""
    r = np.asarray(x).reshape(x.shape[0], 8, 4, 4, 4)            # [row, w, nt, q, r]
    return r.transpose(0, 1, 3, 2, 4).reshape(x.shape[0], 8, 4, 16)


def _row_sum32(v, fma_with=None):
    """The chain's row sum of 512 fp32 values: a lane's chain of 16, shuffles over q (xor 16, xor 32), the tree over the 8 waves.
    fma_with: sum of v * fma_with with one rounding per term (fmaf)."""
    l = _lanes(v)
    m = None if fma_with is None else _lanes(fma_with)
    s = np.zeros(l.shape[:3], dtype=F32)
    for i in range(16):
        s = (s + l[..., i]).astype(F32) if m is None else (s.astype(np.float64) + l[..., i].astype(np.float64) * m[..., i].astype(np.float64)).astype(F32)
    s = ((s[..., 0] + s[..., 1]).astype(F32) + (s[..., 2] + s[..., 3]).astype(F32)).astype(F32)        # [row, w]
    p = s
    return (((p[:, 0] + p[:, 1]).astype(F32) + (p[:, 2] + p[:, 3]).astype(F32)).astype(F32)
            + ((p[:, 4] + p[:, 5]).astype(F32) + (p[:, 6] + p[:, 7]).astype(F32)).astype(F32)).astype(F32)


def ln32(x, g, b, eps=R.EPS, biased=False):
    """y (fp32, before the bf16 rounding), {mean, std} as the chain kernels compute them."""
    x = np.asarray(x, dtype=F32)
    mean = (_row_sum32(x) * F32(1.0 / D)).astype(F32)
    d = (x - mean[:, None]).astype(F32)
    var = (_row_sum32(d, fma_with=d) * F32(1.0 / (D if biased else D - 1))).astype(F32)
    sd = np.sqrt(var).astype(F32)
    rinv = (F32(1.0) / (sd + F32(eps)).astype(F32)).astype(F32)
    y = ((np.asarray(g, F32)[None, :] * d).astype(F32) * rinv[:, None]).astype(F32) + np.asarray(b, F32)[None, :]
    return y.astype(F32), np.stack([mean, sd], 1)


def ln_bwd32(gy, x, st, gain, dres, eps=R.EPS):
    """dx and the block's da / db terms summed over all rows (in fp32, rows in order), as row_bchain_kernel's ln_bwd."""
    gy, x, st = np.asarray(gy, F32), np.asarray(x, F32), np.asarray(st, F32)
    r = (F32(1.0) / (st[:, 1] + F32(eps)).astype(F32)).astype(F32)
    xc = (x - st[:, 0][:, None]).astype(F32)
    ta = ((gy * xc).astype(F32) * r[:, None]).astype(F32)
    da, db = np.zeros(D, F32), np.zeros(D, F32)
    for i in range(gy.shape[0]):
        da, db = (da + ta[i]).astype(F32), (db + gy[i]).astype(F32)
    g = (gy * np.asarray(gain, F32)[None, :]).astype(F32)
    mg = (_row_sum32(g) * F32(1.0 / D)).astype(F32)
    sx = _row_sum32(g, fma_with=xc)
    coef = (((r * r).astype(F32) * sx).astype(F32) / (F32(D - 1) * st[:, 1]).astype(F32)).astype(F32)
    o = ((r[:, None] * (g - mg[:, None]).astype(F32)).astype(F32) - (coef[:, None] * xc).astype(F32)).astype(F32)
    if dres is not None:
        o = (o + np.asarray(dres, F32)).astype(F32)
    return o, da, db


def forward_inputs(p, seed=5, routing=False, M=M_HOST):
    """Inputs and operands of a full chain R L1 S1(3) F L2 S2(3).  The first LayerNorm's input, x_mid, is ln_ref.class_rows: x_in is
    those rows minus the update R adds (float64, rounded once), a_in scaled by the row's class so that the update's own rounding stays
    below the spread of the narrowest class (x_out, the second LayerNorm's input, is of class 0 whatever came in)."""
    g = np.random.default_rng(seed)
    rows, kind = R.class_rows(M, D, seed)
    t = dict(a_in=_bf(g.standard_normal((M, D)) * CLASS_SCALE[kind][:, None]))
    vec = lambda n, sc=0.1: (sc * g.standard_normal(n)).astype(F32)
    w = dict(g1=(1 + vec(D)).astype(F32), b1=vec(D), g2=(1 + vec(D)).astype(F32), b2=vec(D), bias_h=vec(FF), bias_o=vec(D))
    rt = None
    if routing:
        Wr, pr, cr = CR.routing_unit(seed + 1)
        S1, p1, c1 = CR.routing_stack(3, seed + 2)
        W1, ph, ch = CR.routing_stack(NC, seed + 3)
        W2, sg, co = CR.routing_w2(NC, seed + 4)
        S2, p2, c2 = CR.routing_stack(3, seed + 5)
        w.update(Wr=Wr, S1=S1, W1=W1, W2=W2, S2=S2, bias_r=np.zeros(D, F32), bias_s1=np.zeros(3 * D, F32), bias_s2=np.zeros(3 * D, F32))
        rt = dict(Wr=(pr, cr), S1=(p1, c1), W1=(ph, ch), W2=(sg, co), S2=(p2, c2), bias_r=w["bias_r"], bias_h=w["bias_h"], bias_o=w["bias_o"])
    else:
        mk = lambda n, k: _bf(g.standard_normal((n, k)) * (0.5 / np.sqrt(k)))
        w.update(Wr=mk(D, D), S1=mk(3 * D, D), W1=mk(FF, D), W2=mk(D, FF), S2=mk(3 * D, D), bias_r=vec(D), bias_s1=vec(3 * D), bias_s2=vec(3 * D))
    keys = np.arange(M)
    ik = CR.keep_scale(p)
    for site, n in (("r", D), ("h", FF), ("o", D)):
        w["keep_" + site] = (CR.keep(SEEDS[site], keys, n, p) * ik).astype(F32) if p > 0 else np.ones((M, n), F32)
    upd = w["keep_r"].astype(np.float64) * (t["a_in"].astype(np.float64) @ w["Wr"].astype(np.float64).T + w["bias_r"])
    t["x_in"] = (rows.astype(np.float64) - upd).astype(F32)
    return t, w, rt, kind


def emulate_forward(t, w, p, mut=None):
    """The stored tensors of the chain, stage by stage in fp32.  mut: one of the forward MUTANTS."""
    M = t["x_in"].shape[0]
    keys, ik = np.arange(M), CR.keep_scale(p)
    keep_r, keep_h = w["keep_r"], w["keep_h"]
    if mut == "hidden dropout row length 512" and p > 0:
        keep_h = (CR.keep(SEEDS["h"], keys, FF, p, row_len=D) * ik).astype(F32)
    if mut == "partial block keyed as its neighbour" and p > 0:
        k2 = keys.copy(); k2[-3:] += 1                                   # the three rows of a partial last block
        keep_r = (CR.keep(SEEDS["r"], k2, D, p) * ik).astype(F32)
    s = {}
    v = (mm32(t["a_in"], w["Wr"]) + w["bias_r"][None, :]).astype(F32)
    s["x_mid"] = (t["x_in"] + (v * keep_r).astype(F32)).astype(F32)
    y, s["st1"] = ln32(s["x_mid"], w["g1"], w["b1"])
    s["y1"] = _bf(y)
    outs = []
    for i in range(3):
        bias = w["bias_s1"][D * i:D * i + D] if not (mut == "second S1 bias from the first" and i == 1) else w["bias_s1"][:D]
        outs.append(_bf(mm32(s["y1"], w["S1"][D * i:D * i + D], skip_kstep=5 if (mut == "lost k-step" and i == 1) else None) + bias[None, :]))
    s["out1"] = np.concatenate(outs, 1)
    h, acc2 = np.zeros((M, FF), F32), np.zeros((M, D), F32)
    for c in range(NC):
        v = np.maximum((mm32(s["y1"], w["W1"][D * c:D * c + D]) + w["bias_h"][D * c:D * c + D][None, :]).astype(F32), F32(0))
        h[:, D * c:D * c + D] = _bf((v * keep_h[:, D * c:D * c + D]).astype(F32))
        c2 = (c + 1) % NC if mut == "W1 chunk c with W2 chunk c + 1" else c
        hc, wc = h[:, D * c:D * c + D], w["W2"][:, D * c2:D * c2 + D]
        for ks in range(16):
            acc2 = (acc2 + hc[:, 32 * ks:32 * ks + 32] @ wc[:, 32 * ks:32 * ks + 32].T).astype(F32)
    s["h"] = h
    v = (acc2 + w["bias_o"][None, :]).astype(F32)
    s["x_out"] = (s["x_mid"] + (v * w["keep_o"]).astype(F32)).astype(F32)
    y, s["st2"] = ln32(s["x_out"], w["g2"], w["b2"], biased=(mut == "biased std in the second LayerNorm"))
    s["y2"] = _bf(y)
    s["out2"] = np.concatenate([_bf(mm32(s["y2"], w["S2"][D * i:D * i + D]) + w["bias_s2"][D * i:D * i + D][None, :]) for i in range(3)], 1)
    return s


def stages_of(t, s, w, p):
    tt = dict(t); tt.update(s)
    return CR.forward_stages(tt, w, p)


def routing_mismatches(t, s, rt, w):
    tt = dict(t); tt.update(s)
    ex = CR.routing_forward(tt, rt, w)
    return {k: int((np.asarray(s[k], F32) != v).sum()) for k, v in ex.items()}


def backward_inputs(p, seed=9, M=M_HOST):
    g = np.random.default_rng(seed)
    xa, _ = R.class_rows(M, D, seed)
    xb, _ = R.class_rows(M, D, seed + 1)
    mk = lambda n, k: _bf(g.standard_normal((n, k)) * (0.5 / np.sqrt(n)))
    t = dict(ain=_bf(g.standard_normal((M, 3 * D))), xa=xa, xb=xb, dresa=g.standard_normal((M, D)).astype(F32),
             hgate=_bf(np.maximum(g.standard_normal((M, FF)), 0) * (g.random((M, FF)) < 0.9)),
             ca=(0.5 * g.standard_normal((2, D))).astype(F32), cb=(0.5 * g.standard_normal((2, D))).astype(F32))
    w = dict(Win=mk(3 * D, D), W2=mk(D, FF), W1=mk(FF, D), Wo=mk(D, D), ga=(1 + 0.1 * g.standard_normal(D)).astype(F32),
             gb=(1 + 0.1 * g.standard_normal(D)).astype(F32), gate_scale=float(CR.keep_scale(p)))
    keys, ik = np.arange(M), CR.keep_scale(p)
    for site in "ab":
        w["keep_" + site] = (CR.keep(SEEDS[site], keys, D, p) * ik).astype(F32) if p > 0 else np.ones((M, D), F32)
    return t, w


def stats32(x):
    """What the test hands the backward as statistics: the fp32 rounding of the float64 {mean, std}."""
    _, mean, sd = R.forward(x, np.ones(D), np.zeros(D))
    return np.stack([mean, sd], 1).astype(F32)


def emulate_backward(t, w, mut=None, stale=None):
    """The stored tensors of the ZX backward chain in fp32; dresb is the dxa rows this call writes."""
    s = {}
    gy = mm32(t["ain"], np.asarray(w["Win"], F32).T)
    dxa, da, db = ln_bwd32(gy, t["xa"], stats32(t["xa"]), w["ga"], t["dresa"])
    s["dxa"], s["daa"], s["dba"] = dxa, (t["ca"][0] + da).astype(F32), (t["ca"][1] + db).astype(F32)
    s["dza"] = _bf((dxa * w["keep_a"]).astype(F32))
    acc = mm32(s["dza"], np.asarray(w["W2"], F32).T)
    gate = (acc > 0) if mut == "gate from gh" else (t["hgate"] > 0)
    s["gh"] = _bf(np.where(gate, (acc * F32(w["gate_scale"])).astype(F32), F32(0)))
    gy2 = mm32(s["gh"], np.asarray(w["W1"], F32).T)
    dres = stale if mut == "stale dresb" else dxa
    dxb, da, db = ln_bwd32(gy2, t["xb"], stats32(t["xb"]), w["gb"], dres)
    s["dxb"], s["dab"], s["dbb"] = dxb, (t["cb"][0] + da).astype(F32), (t["cb"][1] + db).astype(F32)
    s["dzb"] = _bf((dxb * w["keep_b"]).astype(F32))
    s["out2"] = _bf(mm32(s["dzb"], np.asarray(w["Wo"], F32).T))
    return s


def bstages_of(t, s, w, p):
    tt = dict(t); tt.update(s); tt["dresb"] = s["dxa"]
    return CR.backward_stages(tt, w, workgroups=1, p=p)


# ------------------------------------------------------------------------------------------------ soundness
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_restatement_within_one_bound_forward(p):
    t, w, _, kind = forward_inputs(p)
    s = emulate_forward(t, w, p)
    res = CR.measure(s, stages_of(t, s, w, p))
    print(f"host forward p={p}: error / bound " + ", ".join(f"{k} {v[0]:.4f}" for k, v in res.items()))
    for name, (ratio, n) in res.items():
        assert ratio <= 1.0 and n == 0, (name, ratio, n)
    # ... and on every input class by itself (x_mid, the first LayerNorm's input, keeps the class of x_in)
    st = stages_of(t, s, w, p)
    for k in range(5):
        rows = kind == k
        sub = CR.measure({n: v[rows] for n, v in s.items()}, {n: (r[rows], np.broadcast_to(b, r.shape)[rows]) for n, (r, b) in st.items()})
        print(f"  class {k}: " + ", ".join(f"{n} {v[0]:.4f}" for n, v in sub.items()))
        assert all(v[0] <= 1.0 and v[1] == 0 for v in sub.values()), (k, sub)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_restatement_within_one_bound_backward(p):
    t, w = backward_inputs(p)
    s = emulate_backward(t, w)
    st = bstages_of(t, s, w, p)
    res = CR.measure(s, st)
    print(f"host backward p={p}: error / bound " + ", ".join(f"{k} {v[0]:.4f}" for k, v in res.items()))
    for name, (ratio, n) in res.items():
        assert ratio <= 1.0 and n == 0, (name, ratio, n)
    _, kind = R.class_rows(M_HOST, D, 9)
    rowwise = [n for n in s if s[n].shape[0] == M_HOST and s[n].ndim == 2]
    for k in range(5):           # both LayerNorm inputs of row i are of class i mod 5
        rows = kind == k
        sub = CR.measure({n: s[n][rows] for n in rowwise}, {n: (st[n][0][rows], np.broadcast_to(st[n][1], st[n][0].shape)[rows]) for n in rowwise})
        print(f"  class {k}: " + ", ".join(f"{n} {v[0]:.4f}" for n, v in sub.items()))
        assert all(v[0] <= 1.0 and v[1] == 0 for v in sub.values()), (k, sub)


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_routing_restatement_is_exact(p):
    """The routing chain through the fp32 restatement: every routed output equals its one-term formula, bit for bit."""
    t, w, rt, _ = forward_inputs(p, routing=True)
    s = emulate_forward(t, w, p)
    assert routing_mismatches(t, s, rt, w) == dict(x_mid=0, out1=0, h=0, x_out=0, out2=0)
    sig = rt["W2"][0]
    assert len(set(sig.tolist())) == D and sig.max() < FF, "W2 selects a hidden unit twice"
    assert len({int(x) // D for x in sig}) == NC, "every chunk of W2 carries some output"


def test_bf16_interval_is_at_most_one_neighbour():
    """The interval admits the rounding of the reference and, near a rounding boundary only, its neighbour."""
    g = np.random.default_rng(3)
    ref = g.standard_normal(20000) * 3
    bound = np.abs(ref) * 40 * CR.U
    lo, hi = CR.bf16_rn(ref - 4 * bound).astype(np.float64), CR.bf16_rn(ref + 4 * bound).astype(np.float64)
    step = np.abs(CR.bf16_rn(ref).astype(np.float64)) * 2.0 ** -7
    assert ((hi - lo) <= step * 1.001).all() and ((lo == hi).mean() > 0.95)
    assert CR.interval_miss(CR.bf16_rn(ref), ref, bound) == (0.0, 0)
    up = CR.bf16_rn(ref).astype(np.float64) * (1 + 2.0 ** -7)                  # one step away: outside nearly everywhere
    assert CR.interval_miss(up, ref, bound)[1] > 0.9 * ref.size


# ------------------------------------------------------------------------------------------------ mutants
# name -> (direction, the check that must see it with random operands or None, routed outputs whose bit check must see it or ())
MUTANTS = {
    "lost k-step": ("fwd", "out1", ("out1",)),
    "W1 chunk c with W2 chunk c + 1": ("fwd", "x_out", ("x_out",)),
    "hidden dropout row length 512": ("fwd", "h", ("h",)),
    "partial block keyed as its neighbour": ("fwd", "x_mid", ("x_mid",)),
    "second S1 bias from the first": ("fwd", "out1", ()),                  # routing runs with zero projection biases: blind there
    "biased std in the second LayerNorm": ("fwd", "st2", ()),              # the routed outputs take the stored y2: blind there
    "gate from gh": ("bwd", "gh", ()),
    "stale dresb": ("bwd", "dxb", ()),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant(name):
    direction, seen_by, routed = MUTANTS[name]
    p = 0.5 if "dropout" in name or "keyed" in name else 0.1
    if direction == "fwd":
        t, w, _, _ = forward_inputs(p)
        s = emulate_forward(t, w, p, mut=name)
        res = CR.measure(s, stages_of(t, s, w, p))
        t2, w2, rt, _ = forward_inputs(0.5, routing=True)
        mism = routing_mismatches(t2, emulate_forward(t2, w2, 0.5, mut=name), rt, w2)
    else:
        t, w = backward_inputs(p)
        s = emulate_backward(t, w, mut=name, stale=np.zeros((M_HOST, D), F32))
        res = CR.measure(s, bstages_of(t, s, w, p))
        mism = {}
        if name == "stale dresb":        # the GPU file's buffers start as NaN: there the finiteness assertion sees it first
            sn = emulate_backward(t, w, mut=name, stale=np.full((M_HOST, D), np.nan, F32))
            assert not np.isfinite(sn["dxb"]).any()
    print(f"mutant {name!r}: " + ", ".join(f"{k} {v[0]:.3g} ({v[1]} out)" for k, v in res.items()) + f"; routing mismatches {mism}")
    ratio, n = res[seen_by]
    assert n > 0 and (ratio > CR.MARGIN or seen_by not in CR.FP32_OUTPUTS), (name, seen_by, ratio, n)
    # every other stage is computed from the stored inputs: the mutant shows in ITS stage alone (and y2 for the std, a rounding of it)
    for k, (r2, n2) in res.items():
        if k != seen_by and not (name.startswith("biased") and k == "y2"):
            assert n2 == 0, (name, k, r2, n2)
    for k in routed:
        assert mism[k] > 0, (name, k)
    for k, v in mism.items():
        if k not in routed:
            assert v == 0, (name, k, v)


def test_dropout_mutants_are_invisible_without_dropout():
    """The two dropout-index mutants change nothing at p = 0: the GPU cases that see them are the p > 0 ones (stated, not hidden)."""
    t, w, _, _ = forward_inputs(0.0)
    ref = emulate_forward(t, w, 0.0)
    for name in ("hidden dropout row length 512", "partial block keyed as its neighbour"):
        s = emulate_forward(t, w, 0.0, mut=name)
        assert all(np.array_equal(s[k], ref[k]) for k in ref)


# ------------------------------------------------------------------------------------------------ geometry against the plan query
@pytest.fixture(scope="module")
def L():
    import sparse_image_captioning_amd as P
    return P._lib


def chain_args(L, M, parts="R1S3FL2S3", nc=NC, progress=False, ld_pad=0):
    """ortk_chain_args with placeholder pointers (the plan tests them for NULL only)."""
    P_ = 4096
    a = L.ChainArgs()
    hasR, hasF = "R" in parts, "F" in parts
    n1 = int(parts[parts.index("1S") + 2]) if "1S" in parts else 0
    n2 = int(parts[parts.index("2S") + 2]) if "2S" in parts else 0
    a.n_units = (1 if hasR else 0) + n1 + (2 * nc if hasF else 0) + n2
    a.w16, a.units_dev, a.packed, a.packed_bytes = P_, P_, P_, L.lib().ortk_chain_packed_bytes(a.n_units)
    a.M, a.x_in = M, P_
    if hasR: a.a_in, a.bias_r, a.x_mid = P_, P_, P_
    a.g1, a.b1, a.y1, a.st1 = P_, P_, P_, P_
    a.n1 = n1
    if n1: a.bias_s1, a.out1, a.ld1 = P_, P_, n1 * D + ld_pad
    if hasF: a.NC, a.bias_h, a.bias_o, a.h, a.x_out = nc, P_, P_, P_, P_
    if "L2" in parts: a.g2, a.b2, a.y2, a.st2 = P_, P_, P_, P_
    a.n2 = n2
    if n2: a.bias_s2, a.out2, a.ld2 = P_, P_, n2 * D + ld_pad
    a.drop_p, a.eps = 0.1, 1e-6
    if progress: a.progress = P_
    return a


def bchain_args(L, M, kind="ZX"):
    P_ = 4096
    a = L.BChainArgs()
    nin = {"ZX": 3, "X": 0, "Y": 1, "Z": 3}[kind]
    hasF, n2 = kind in ("ZX", "X"), (0 if kind == "Z" else 1)
    a.n_units = nin + (2 * NC if hasF else 0) + n2
    a.w16t, a.units_dev, a.packed, a.packed_bytes, a.M = P_, P_, P_, L.lib().ortk_chain_packed_bytes(a.n_units), M
    a.nin = nin
    if nin:
        a.ain, a.ld_ain, a.xa, a.sta, a.ga, a.dresa, a.dxa, a.daa, a.dba, a.dza = P_, nin * D, P_, P_, P_, P_, P_, P_, P_, P_
        a.mask_a = 0 if kind == "Z" else 1
    else:
        a.dz0 = P_
    if hasF:
        a.NC, a.hgate, a.gh, a.gate_scale, a.xb, a.stb, a.gb, a.dresb, a.dxb, a.dab, a.dbb, a.mask_b, a.dzb = NC, P_, P_, 1.0, P_, P_, P_, P_, P_, P_, P_, 1, P_
    a.n2 = n2
    if n2: a.out2 = P_
    a.drop_p, a.eps = 0.1, 1e-6
    return a


def _plan_keys(d):
    return {k: d[k] for k in ("form", "rows_per_block", "workgroups", "prefetchers")}


def test_case_table_against_restatement_and_plan(L):
    old = L.set_tuning()
    try:
        seen = set()
        for (M, cw, pf), (form, rb, wg, last) in CR.GEOMETRY_CASES.items():
            L.set_tuning(chain_wide=cw)
            g = CR.plan(M, cw, bool(pf))
            assert (g["form"], g["rows_per_block"], g["workgroups"], g["last"]) == (form, rb, wg, last), (M, cw, pf, g)
            assert L.row_chain_plan(chain_args(L, M, progress=bool(pf))) == _plan_keys(g), (M, cw, pf)
            seen |= CR.geometry_classes(M, cw, bool(pf))
            print(f"plan M={M} chain_wide={cw} progress={pf}: form {form} rb {rb} workgroups {wg} last block {last} prefetchers {g['prefetchers']}")
        assert CR.ALL_CLASSES <= seen, CR.ALL_CLASSES - seen
        # M = 24 577 is the smallest row count with two wide rounds against three narrow ones
        assert CR.is_wide(24577, 2) and CR.plan(24577, 2)["rounds"] == 2 and not any(CR.plan(m, 2)["rounds"] == 2 and CR.is_wide(m, 2) for m in range(19457, 24577))
        # rb = 48 is not reached below 11 657 rows (248 slots; 12 033 with 256), the wide form not below 12 289: why the tall cases exist
        assert min(m for m in range(1, 12289) if CR.rows_per_block(m, 248) == 48) == 11657
        assert min(m for m in range(1, 12289) if CR.rows_per_block(m) == 48) == 12033 and not any(CR.is_wide(m) for m in range(1, 12289))
    finally:
        L.set_tuning(**old)
    for M in CR.BWD_ROWS:
        g = CR.bplan(M)
        for kind in ("ZX", "X", "Y", "Z"):
            assert L.row_bchain_plan(bchain_args(L, M, kind)) == {k: g[k] for k in ("rows_per_block", "workgroups")}


def test_geometry_sweep_against_plan(L):
    """M = 1 .. 40 000 in steps that include every multiple of 248 and 256 and their neighbours, every tuning value, with and without
    prefetchers; the shortest and the longest chain (the geometry does not depend on the parts)."""
    Ms = set(range(1, 600)) | set(range(11600, 12400)) | set(range(19400, 19500)) | set(range(24500, 24600)) | set(range(1, 40001, 97))
    for k in (248, 256):
        for m in range(k, 40001, k):
            Ms |= {m - 1, m, m + 1}
    Ms = sorted(m for m in Ms if 1 <= m <= 40000)
    old = L.set_tuning()
    try:
        for cw in (0, 1, 2):
            L.set_tuning(chain_wide=cw)
            for pf in (False, True):
                a, b = chain_args(L, 1, progress=pf), chain_args(L, 1, parts="1S1", progress=pf)
                for M in Ms:
                    a.M = b.M = M
                    want = _plan_keys(CR.plan(M, cw, pf))
                    assert L.row_chain_plan(a) == want and L.row_chain_plan(b) == want, (M, cw, pf)
    finally:
        L.set_tuning(**old)
    ba = bchain_args(L, 1)
    for M in Ms:
        ba.M = M
        g = CR.bplan(M)
        assert L.row_bchain_plan(ba) == {k: g[k] for k in ("rows_per_block", "workgroups")}, M


def test_plan_refusals(L):
    EINVAL = -1
    f = lambda a: L.lib().ortk_row_chain_plan(C.byref(a), None, None, None, None)
    fb = lambda a: L.lib().ortk_row_bchain_plan(C.byref(a), None, None)
    assert f(chain_args(L, 1000)) == 0 and fb(bchain_args(L, 1000)) == 0
    a = chain_args(L, 1000); a.n_units += 1; a.packed_bytes = L.lib().ortk_chain_packed_bytes(a.n_units); assert f(a) == EINVAL     # n_units against the parts
    a = chain_args(L, 1000); a.ld1 = 3 * D - 4; assert f(a) == EINVAL
    a = chain_args(L, 1000); a.ld2 = 3 * D + 2; assert f(a) == EINVAL                                                    # not a multiple of 4
    a = chain_args(L, 1000, nc=9); assert f(a) == EINVAL
    a = chain_args(L, 1000, nc=8); assert f(a) == 0
    a = chain_args(L, 1000); a.drop_p = 1.0; assert f(a) == EINVAL
    a = chain_args(L, 1000); a.packed_bytes -= 1; assert f(a) == EINVAL
    a = chain_args(L, 1000); a.x_in = None; assert f(a) == EINVAL
    a = chain_args(L, 1000); a.M = 0; assert f(a) == EINVAL
    a = chain_args(L, 1000, ld_pad=8); assert f(a) == 0
    assert L.lib().ortk_row_chain_plan(None, None, None, None, None) == EINVAL and L.lib().ortk_row_bchain_plan(None, None, None) == EINVAL
    b = bchain_args(L, 1000); b.nin = 2; b.n_units -= 1; b.ld_ain = 2 * D; assert fb(b) == EINVAL
    b = bchain_args(L, 1000, "Y"); b.mask_a = 0; assert fb(b) == EINVAL                                                  # mask_a = 0 with n2 = 1
    b = bchain_args(L, 1000); b.packed_bytes -= 1; assert fb(b) == EINVAL
    b = bchain_args(L, 1000); b.drop_p = 1.0; assert fb(b) == EINVAL
    with pytest.raises(L.OrtkError):
        L.row_chain_plan(chain_args(L, 1000, nc=9))
