"""The LayerNorm error model of tests/ln_ref.py, checked on the CPU: the bars tests/test_gpu_layernorm.py asserts are sound (an fp32
restatement of the kernels' own arithmetic stays within ONE bound on every input class and width) and sharp (each natural slip of a
rewrite exceeds the asserted FOUR bounds on some class).  Run with -s for the tables (profiles/layernorm_operator_tests.txt).

The restatement follows csrc/ortk_norm.hip operation by operation in numpy float32: lane l owns columns 4 l .. 4 l + 3 (+ 256 it) in
the vector form and l (+ 64 it) in the scalar form, sums its NREG values in a chain, the 64 lanes combine in six butterfly levels;
two passes over the row, rinv = 1 / (sd + eps); the backward's column sums run rows_per_block / 4 rows per wave in a chain, the four
waves as (w0 + w1) + (w2 + w3), one add per block onto what the output held."""
import numpy as np
import pytest
import torch

import ln_ref as R

F = np.float32
FWD_D = (2, 3, 8, 63, 65, 508, 510, 512, 513, 516, 1030, 2044, 2047, 2048)      # every width of tests/test_gpu_layernorm.py
BWD_D = (2, 3, 6, 8, 100, 510, 512, 516, 1030, 2044, 2047, 2048)
CLASS_NAME = {0: "2 randn", 1: "1024 + 2 randn", 2: "1e-3 randn", 3: "1e-6 randn", 4: "1 + 1e-3 randn", 5: "constant 1.5"}
FWD_MUTANTS = ("one_pass", "biased", "eps_in_root")
BWD_MUTANTS = ("no_mean_g", "coef_d", "da_no_r")
MUTANT_D = (3, 8, 100, 512, 516, 1030, 2048)      # a width of every kernel instance
SEEN_UP_TO = {"coef_d": 1030}
LANES = np.arange(64)


def _lane_cols(d):
    """(NREG, 64) column owned by slot i of lane l (-1: past the row): the vector form where d % 4 == 0, else the scalar form."""
    n = R.nreg(d)
    i = np.arange(n)[:, None]
    cols = (LANES[None, :] * 4 + 256 * (i // 4) + i % 4) if d % 4 == 0 else (LANES[None, :] + 64 * i)
    return np.where(cols < d, cols, -1)


def _row_sum(v):
    """v (rows, NREG, 64) float32, zeros in the slots past the row: the lane chains, then wave_sum's butterfly."""
    s = np.zeros((v.shape[0], 64), F)
    for i in range(v.shape[1]):
        s = s + v[:, i, :]
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, LANES ^ o]
    return s[:, 0]


def _spread(t, cols):
    return np.where(cols >= 0, t[:, np.maximum(cols, 0)], F(0))


def restated_forward(x, a, b, eps=R.EPS, mutant=None):
    x, a, b, eps = x.astype(F), a.astype(F), b.astype(F), F(eps)
    d = x.shape[1]
    cols = _lane_cols(d)
    v = _spread(x, cols)
    mean = _row_sum(v) / F(d)
    if mutant == "one_pass":
        q = np.maximum(_row_sum(v * v) - F(d) * mean * mean, F(0))
    else:
        t = np.where(cols >= 0, v - mean[:, None, None], F(0))
        q = _row_sum(t * t)
    var = q / F(d if mutant == "biased" else d - 1)
    sd = np.sqrt(var)
    rinv = F(1) / np.sqrt(var + eps) if mutant == "eps_in_root" else F(1) / (sd + eps)
    y = a * (x - mean[:, None]) * rinv[:, None] + b
    return y, mean, sd


def restated_backward(dy, x, a, mean, sd, eps=R.EPS, dres=None, ca=None, cb=None, rpb=None, mutant=None, skip_row=None):
    dy, x, a, mean, sd, eps = dy.astype(F), x.astype(F), a.astype(F), mean.astype(F), sd.astype(F), F(eps)
    rows, d = x.shape
    cols = _lane_cols(d)
    r = F(1) / (sd + eps)
    xc = x - mean[:, None]
    g = dy * a
    sg, sgx = _row_sum(_spread(g, cols)), _row_sum(_spread(g * xc, cols))
    mg = np.zeros_like(sg) if mutant == "no_mean_g" else sg / F(d)
    coef = r * r * sgx / (F(d if mutant == "coef_d" else d - 1) * sd)
    dx = r[:, None] * (g - mg[:, None]) - coef[:, None] * xc
    if dres is not None:
        dx = dx + dres.astype(F)
    ta = dy * xc if mutant == "da_no_r" else dy * xc * r[:, None]
    rpb = R.rows_per_block(rows) if rpb is None else rpb
    da = np.zeros(d, F) if ca is None else ca.astype(F).copy()
    db = np.zeros(d, F) if cb is None else cb.astype(F).copy()
    for r0 in range(0, rows, rpb):
        pa, pb = np.zeros((4, d), F), np.zeros((4, d), F)
        for rr in range(min(rpb, rows - r0)):
            if r0 + rr == skip_row:
                continue
            pa[rr % 4] = pa[rr % 4] + ta[r0 + rr]
            pb[rr % 4] = pb[rr % 4] + dy[r0 + rr]
        da = da + ((pa[0] + pa[1]) + (pa[2] + pa[3]))
        db = db + ((pb[0] + pb[1]) + (pb[2] + pb[3]))
    return dx, da, db


def _params(d, seed):
    g = np.random.default_rng(seed)
    return (1 + 0.1 * g.standard_normal(d)).astype(F), (0.1 * g.standard_normal(d)).astype(F)


def _forward_ratios(d, mutant=None, rows=24):
    """{class: largest error / bound over y, mean, sd} of the restatement at width d."""
    x, kind = R.class_rows(rows, d, 1000 + d, R.FWD_CLASSES)
    a, b = _params(d, 7 + d)
    y, mean, sd = restated_forward(x, a, b, mutant=mutant)
    ry, rm, rs = R.forward(x, a, b)
    by, bm, bs = R.forward_bound(x, a, b)
    out = {}
    for k in np.unique(kind):
        m = kind == k
        if mutant == "eps_in_root":      # (a rewrite with the eps inside the root still reports sqrt(var): y is what it gets wrong)
            out[int(k)] = R.ratio(np.abs(y[m] - ry[m]), by[m])
        else:
            out[int(k)] = max(R.ratio(np.abs(y[m] - ry[m]), by[m]), R.ratio(np.abs(mean[m] - rm[m]), bm[m]), R.ratio(np.abs(sd[m] - rs[m]), bs[m]))
    return out


def _backward_case(d, rows, seed):
    x, kind = R.class_rows(rows, d, seed, R.BWD_CLASSES)
    g = np.random.default_rng(seed + 1)
    a, _ = _params(d, seed + 2)
    dy, dres = g.standard_normal((rows, d)).astype(F), g.standard_normal((rows, d)).astype(F)
    ca, cb = g.standard_normal(d).astype(F), g.standard_normal(d).astype(F)
    return x, kind, a, dy, dres, ca, cb


def _backward_ratios(d, mutant=None, rows=20):
    """{class: dx error / bound}, da error / bound, db error / bound of the restatement at width d (stats from the restated forward)."""
    x, kind, a, dy, dres, ca, cb = _backward_case(d, rows, 2000 + d)
    _, mean, sd = restated_forward(x, a, np.zeros(d, F))
    dx, da, db = restated_backward(dy, x, a, mean, sd, dres=dres, ca=ca, cb=cb, mutant=mutant)
    rdx, rda, rdb = R.backward(dy, x, a, dres=dres)
    bdx, ea, ta, eb, tb = R.backward_bound(dy, x, a, dres=dres)
    lv, nb = R.colsum_shape(rows)
    out = {int(k): R.ratio(np.abs(dx[kind == k] - rdx[kind == k]), bdx[kind == k]) for k in np.unique(kind)}
    return (out, R.ratio(np.abs(da - (ca.astype(np.float64) + rda)), R.colsum_bound(ea, ta, lv, nb, ca)),
            R.ratio(np.abs(db - (cb.astype(np.float64) + rdb)), R.colsum_bound(eb, tb, lv, nb, cb)))


def test_reference_is_the_autograd_of_the_reference_module():
    """ln_ref.forward / backward against torch float64 autograd of a (x - mean) / (std_unbiased + eps) + b."""
    for d in (2, 3, 100, 512):
        x, kind, a, dy, dres, _, _ = _backward_case(d, 10, 50 + d)
        b = _params(d, 3)[1]
        xt, at, bt = (torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in (x, a, b))
        yt = at * (xt - xt.mean(-1, keepdim=True)) / (xt.std(-1, keepdim=True) + R.EPS) + bt
        yt.backward(torch.tensor(dy, dtype=torch.float64))
        y, mean, sd = R.forward(x, a, b)
        dx, da, db = R.backward(dy, x, a, dres=dres)
        scale = lambda t: 1e-11 * max(1.0, float(np.abs(t).max()))
        assert np.abs(y - yt.detach().numpy()).max() <= scale(y)
        assert np.abs(mean - xt.mean(-1).detach().numpy()).max() <= scale(mean) and np.abs(sd - xt.std(-1).detach().numpy()).max() <= scale(sd)
        assert np.abs(dx - dres - xt.grad.numpy()).max() <= scale(dx)
        assert np.abs(da - at.grad.numpy()).max() <= scale(da) and np.abs(db - bt.grad.numpy()).max() <= scale(db)


def test_constant_rows_are_exact_in_reference_and_restatement():
    for d in (3, 512, 2047):
        x = np.full((2, d), 1.5, F)
        a, b = _params(d, d)
        for y, mean, sd in (R.forward(x, a, b), restated_forward(x, a, b)):
            assert (y == b).all() and (mean == 1.5).all() and (sd == 0).all()


@pytest.mark.parametrize("d", FWD_D)
def test_forward_restatement_within_one_bound(d):
    r = _forward_ratios(d)
    print(f"ln host fwd d={d:5d}: " + "  ".join(f"{CLASS_NAME[k]}: {v:.4f}" for k, v in sorted(r.items())))
    assert set(r) == set(R.FWD_CLASSES) and max(r.values()) <= 1.0


@pytest.mark.parametrize("d", BWD_D)
def test_backward_restatement_within_one_bound(d):
    r, ra, rb = _backward_ratios(d)
    print(f"ln host bwd d={d:5d}: " + "  ".join(f"{CLASS_NAME[k]}: {v:.4f}" for k, v in sorted(r.items())) + f"  da: {ra:.4f}  db: {rb:.4f}")
    assert set(r) == set(R.BWD_CLASSES) and max(r.values()) <= 1.0 and ra <= 1.0 and rb <= 1.0


def test_tall_column_sums_within_one_bound():
    """The 64-rows-per-block height and its 257 block adds, at the width of the tall GPU cases."""
    rows, d = 16387, 8
    x, kind, a, dy, dres, ca, cb = _backward_case(d, rows, 77)
    _, mean, sd = restated_forward(x, a, np.zeros(d, F))
    dx, da, db = restated_backward(dy, x, a, mean, sd, ca=ca, cb=cb)
    rdx, rda, rdb = R.backward(dy, x, a)
    bdx, ea, ta, eb, tb = R.backward_bound(dy, x, a)
    lv, nb = R.colsum_shape(rows)
    assert (lv, nb) == (18, 257)
    ra = R.ratio(np.abs(da - (ca.astype(np.float64) + rda)), R.colsum_bound(ea, ta, lv, nb, ca))
    rb = R.ratio(np.abs(db - (cb.astype(np.float64) + rdb)), R.colsum_bound(eb, tb, lv, nb, cb))
    print(f"ln host bwd rows={rows} d={d}: dx {R.ratio(np.abs(dx - rdx), bdx):.4f}  da {ra:.4f}  db {rb:.4f}")
    assert R.ratio(np.abs(dx - rdx), bdx) <= 1.0 and ra <= 1.0 and rb <= 1.0


def _mutant_line(mutant, d, r, extra=""):
    return f"ln host mutant {mutant:12s} d={d:5d}: " + "  ".join(f"{CLASS_NAME[k]}: {v:.3g}" for k, v in sorted(r.items())) + extra


@pytest.mark.parametrize("mutant", FWD_MUTANTS)
def test_forward_mutant_exceeds_four_bounds(mutant):
    """At every width of MUTANT_D the mutated forward is more than 4 bounds off on some class."""
    for d in MUTANT_D:
        r = _forward_ratios(d, mutant)
        print(_mutant_line(mutant, d, r))
        assert max(v for k, v in r.items() if k != 5) > R.MARGIN, d


@pytest.mark.parametrize("mutant", BWD_MUTANTS)
def test_backward_mutant_exceeds_four_bounds(mutant):
    """The same for the backward (dx; da for the mutant of da).  `coef` with d for d - 1 is a relative change of 1 / d of one term of
    dx: from about 2 000 columns on it is within four worst-case fp32 bounds of the correct value (printed, not asserted), so the
    GPU cases that carry this check for the NREG = 32 instances are the ones at d = 516 and 1030."""
    for d in MUTANT_D:
        r, ra, _ = _backward_ratios(d, mutant)
        print(_mutant_line(mutant, d, r, f"  da: {ra:.3g}"))
        if d <= SEEN_UP_TO.get(mutant, max(MUTANT_D)):
            assert (ra if mutant == "da_no_r" else max(r.values())) > R.MARGIN, d


def test_one_pass_variance_needs_the_large_offset():
    """Why class 1 sits at 1024: at an offset of 64 a one-pass variance is still near the bar, at 1024 far beyond it."""
    out = {}
    for off in (64.0, 1024.0):
        worst = np.inf
        for d in (8, 100, 512, 2048):
            g = np.random.default_rng(int(off) + d)
            x = (off + 2.0 * g.standard_normal((8, d))).astype(F)
            a, b = _params(d, d)
            y, _, _ = restated_forward(x, a, b, mutant="one_pass")
            worst = min(worst, R.ratio(np.abs(y - R.forward(x, a, b)[0]), R.forward_bound(x, a, b)[0]))
        out[off] = worst
    print(f"ln host one-pass variance, smallest y error / bound over d: offset 64: {out[64.0]:.3g}   offset 1024: {out[1024.0]:.3g}")
    assert out[1024.0] > R.MARGIN and out[1024.0] > 4 * out[64.0]


@pytest.mark.parametrize("d", (6, 8, 512))
def test_a_dropped_row_of_the_column_sums_is_seen(d):
    """rows = 37 (one block of 32 and one of 5): leaving any single row out of da / db moves some column by more than 4 bounds."""
    rows = 37
    x, kind, a, dy, dres, ca, cb = _backward_case(d, rows, 300 + d)
    _, mean, sd = restated_forward(x, a, np.zeros(d, F))
    rdx, rda, rdb = R.backward(dy, x, a)
    bdx, ea, ta, eb, tb = R.backward_bound(dy, x, a)
    lv, nb = R.colsum_shape(rows)
    ba, bb = R.colsum_bound(ea, ta, lv, nb, ca), R.colsum_bound(eb, tb, lv, nb, cb)
    seen = 0
    for k in range(rows):
        _, da, db = restated_backward(dy, x, a, mean, sd, ca=ca, cb=cb, skip_row=k)
        hit = max(R.ratio(np.abs(da - (ca.astype(np.float64) + rda)), ba), R.ratio(np.abs(db - (cb.astype(np.float64) + rdb)), bb)) > R.MARGIN
        seen += hit
    print(f"ln host dropped row, rows={rows} d={d}: seen {seen} of {rows}")
    assert seen == rows


def test_share_of_dropped_rows_seen_at_the_tall_case():
    """At 16 387 rows the column sums' bound has grown with the row count: the share of single dropped rows that still move a
    column of da (of db) by more than 4 bounds, from the reference's own terms.  da carries the per-term error of 16 387 rows and
    sees no single row any more; db (exact terms, the summation error only) still sees nearly every one.  The cases of 37 rows
    above carry the check for da."""
    rows = 16387
    for d in (8, 512):
        x, kind, a, dy, _, ca, cb = _backward_case(d, rows, 400 + d)
        bdx, ea, ta, eb, tb = R.backward_bound(dy, x, a)
        lv, nb = R.colsum_shape(rows)
        ba, bb = R.colsum_bound(ea, ta, lv, nb, ca), R.colsum_bound(eb, tb, lv, nb, cb)
        xd = x.astype(np.float64)
        xc = xd - xd.mean(-1, keepdims=True)
        r = 1.0 / (np.sqrt((xc * xc).sum(-1) / (d - 1)) + R.EPS)
        sa = (np.abs(dy * xc * r[:, None]) > R.MARGIN * ba).any(-1).mean()
        sb = (np.abs(dy.astype(np.float64)) > R.MARGIN * bb).any(-1).mean()
        print(f"ln host dropped row, rows={rows} d={d}: share seen through da {sa:.4f}, through db {sb:.4f}")
        assert sa <= 0.01 and sb >= 0.9
