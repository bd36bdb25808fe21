"""Float64 reference and fp32 error model of the project's LayerNorm (csrc/ortk_norm.hip, the two ln_mode epilogues of csrc/ortk_gemm.hip).
numpy only, no GPU.  tests/test_ln_ref_host.py shows on the CPU that the bars below are sound and sharp; tests/test_gpu_layernorm.py
holds the kernels to them.

The operator is the reference's non-standard LayerNorm (models/transformer.py: LayerNorm.forward), per row of n = d values:

    mean = sum(x) / n        xc = x - mean        q = sum(xc^2)        sd = sqrt(q / (n - 1))        r = 1 / (sd + eps)
    y  = a xc r + b
    g  = dy a      sg = sum(g)      sgx = sum(g xc)      mg = sg / n      coef = r^2 sgx / ((n - 1) sd)
    dx = r (g - mg) - coef xc  [+ dres]            da += sum_rows dy xc r            db += sum_rows dy

(unbiased std, eps OUTSIDE the root).  `forward` and `backward` evaluate exactly this in float64 from x itself; the backward never
sees the kernel's statistics.

Error model.  u = 2^-24 (the unit roundoff of fp32), D = the additions on the longest path of a row sum, read off the kernel:

    ortk_norm.hip       a lane's chain of NREG terms (8 for d <= 512, 32 above), six shuffle levels, the division:  D = NREG + 7
    gemm_bf16_row512    32 values per lane, two shuffles, two levels over the four column waves, the scaling:        D = 37
    gemm_bf16_rowln_bwd 16 values per lane, two shuffles, three levels over the eight column waves, the scaling:    D = 22

Every quantity below is a per-entry (per-row for the statistics) bound on |fp32 value - float64 value|, worst case and linear in the
number of terms; |.| of a float64 quantity, sums over the row:

    d_mean = D u sum|x| / n
    d_xc   = u |xc| + d_mean
    d_q    = sum (2 |xc| d_xc + d_xc^2) + D u q
    d_sd   = sd (d_q / 2q + 2u)                          (q = 0, a constant row: sqrt(d_q / (n - 1)))
    d_r/r  = d_sd / (sd + eps) + 2u
    d_y    = |a| r (d_xc + |xc| (d_r/r + 3u)) + u |y|

The backward is handed the forward's statistics, so it starts from d_mean, d_sd (hence d_xc, d_r/r) above; e = a bound on the error
its dy already carries (0 for a stored tensor, the product's (K + 2) u sum|a||w| in the fused kernel):

    d_g    = u |g| + |a| e
    d_sg   = sum d_g + D u sum|g|                         d_mg = d_sg / n + u |mg|
    d_t    = |g| d_xc + |xc| d_g + u |g xc|               d_sgx = sum d_t + D u sum|g xc|
    d_coef = |coef| (2 d_r/r + d_sd / sd + 4u) + r^2 d_sgx / ((n - 1) sd)
    d_dx   = r (d_g + d_mg + u |g - mg|) + |r (g - mg)| (d_r/r + u) + |coef| d_xc + |xc| d_coef + u |coef xc|
             + u |r (g - mg) - coef xc| + u |dx|          (+ u |dx + dres| with a residual gradient)
    da term  t = dy xc r:  d_t = |dy| r d_xc + |t| (d_r/r + 2u) + e |xc| r            db term  t = dy:  d_t = e

da / db are column sums over all rows.  A block of `rpb` rows (32; 64 from 16 384 rows on) sums rpb / 4 rows per wave in a chain, the
four waves in two levels, and adds the block's sum to the output with one float atomic (the fused kernel: MT rows in a chain, four
DPP levels, one atomic per workgroup); every atomic rounds at the running value, and the output held c before the call:

    bound = sum_rows d_t + (chain + levels + nblocks) u sum_rows |t| + nblocks u |c|

Every comparison asserts |kernel - reference| <= MARGIN x bound with MARGIN = 4: the margin for the compiler's reassociation and
contraction and for the rounding of the division.  No bar is derived from what a kernel returns.  Outputs that are a rounding or a
masked copy of another output of the same kernel (bf16 y, dz) are compared exactly, with no bar.

Input classes (class_rows): the model must stay sound, and the mutants of tests/test_ln_ref_host.py visible, on
    0  2 randn                     the data of the older tests
    1  1024 + 2 randn              a one-pass variance cancels catastrophically here
    2  1e-3 randn                  sd << 1: eps inside the root, or applied twice, shows
    3  1e-6 randn                  sd about eps
    4  1 + 1e-3 randn              class 2 with an offset
    5  the constant 1.5            forward only: y == b, sd == 0, mean == 1.5 exactly.  The backward of a constant row is 0 / 0 (NaN) in
                                   the reference as well (the gradient of std at q = 0), so no backward case contains one."""
import numpy as np

U = 2.0 ** -24
MARGIN = 4.0
EPS = 1e-6
D_ROW512 = 37          # gemm_bf16_row512_kernel's row sums
D_ROWLN_BWD = 22       # gemm_bf16_rowln_bwd_kernel's row sums
FWD_CLASSES = (0, 1, 2, 3, 5, 4)       # row i of a forward case is of class FWD_CLASSES[i % 6]: four rows hold classes 0 - 3
BWD_CLASSES = (0, 1, 2, 3, 4)          # ... of a backward case BWD_CLASSES[i % 5]
CHUNK = 2048                           # rows per pass of the bound computations (bounds the float64 temporaries of the tall cases)


def nreg(d):
    """Floats per lane of the standalone kernels (ortk_norm.hip: NREG)."""
    return 8 if d <= 512 else 32


def depth(d):
    """D of the standalone kernels' row sums at width d."""
    return nreg(d) + 7


def rows_per_block(rows):
    """Rows a workgroup of the standalone backward walks (ortk_layernorm_bwd_dt)."""
    return 64 if rows >= 16384 else 32


def colsum_shape(rows):
    """(chain + levels, nblocks) of the standalone backward's da / db sums."""
    rpb = rows_per_block(rows)
    return rpb // 4 + 2, -(-rows // rpb)


def class_rows(rows, d, seed, classes=BWD_CLASSES):
    """(rows, d) fp32 inputs, row i of class classes[i % len(classes)]."""
    g = np.random.default_rng(seed)
    z = g.standard_normal((rows, d))
    x = np.empty((rows, d))
    kind = np.array([classes[i % len(classes)] for i in range(rows)])
    for k, (off, scale) in enumerate([(0.0, 2.0), (1024.0, 2.0), (0.0, 1e-3), (0.0, 1e-6), (1.0, 1e-3), (1.5, 0.0)]):
        x[kind == k] = off + scale * z[kind == k]
    return x.astype(np.float32), kind


def _f64(t):
    return np.asarray(t, dtype=np.float64)


def forward(x, a, b, eps=EPS):
    """y (rows, d), mean (rows), sd (rows) in float64."""
    x, a, b = _f64(x), _f64(a), _f64(b)
    n = x.shape[-1]
    mean = x.sum(-1) / n
    xc = x - mean[:, None]
    sd = np.sqrt((xc * xc).sum(-1) / (n - 1))
    return a * xc / (sd + eps)[:, None] + b, mean, sd


def backward(dy, x, a, eps=EPS, dres=None):
    """dx (rows, d), da (d), db (d) in float64, from x itself."""
    dy, x, a = _f64(dy), _f64(x), _f64(a)
    n = x.shape[-1]
    mean = x.sum(-1) / n
    xc = x - mean[:, None]
    sd = np.sqrt((xc * xc).sum(-1) / (n - 1))
    r = 1.0 / (sd + eps)
    g = dy * a
    mg = g.sum(-1) / n
    coef = r * r * (g * xc).sum(-1) / ((n - 1) * sd)
    dx = r[:, None] * (g - mg[:, None]) - coef[:, None] * xc
    if dres is not None:
        dx = dx + _f64(dres)
    return dx, (dy * xc * r[:, None]).sum(0), dy.sum(0)


def _stats_model(x, eps, D):
    """xc, sd, r and the bounds d_mean, d_xc, d_sd, d_r/r of one chunk of rows."""
    n = x.shape[-1]
    mean = x.sum(-1) / n
    xc = x - mean[:, None]
    q = (xc * xc).sum(-1)
    sd = np.sqrt(q / (n - 1))
    r = 1.0 / (sd + eps)
    d_mean = D * U * np.abs(x).sum(-1) / n
    d_xc = U * np.abs(xc) + d_mean[:, None]
    d_q = (2.0 * np.abs(xc) * d_xc + d_xc * d_xc).sum(-1) + D * U * q
    with np.errstate(divide="ignore", invalid="ignore"):
        d_sd = np.where(q > 0, sd * (d_q / (2.0 * q) + 2.0 * U), np.sqrt(d_q / (n - 1)))
    d_rr = d_sd / (sd + eps) + 2.0 * U
    return xc, sd, r, d_mean, d_xc, d_sd, d_rr


def forward_bound(x, a, b, eps=EPS, D=None):
    """Bounds of y (rows, d), mean (rows), sd (rows) under the model; D defaults to the standalone kernels'."""
    x, a, b = _f64(x), _f64(a), _f64(b)
    D = depth(x.shape[-1]) if D is None else D
    by, bm, bs = [], [], []
    for s in range(0, x.shape[0], CHUNK):
        xc, sd, r, d_mean, d_xc, d_sd, d_rr = _stats_model(x[s:s + CHUNK], eps, D)
        y = a * xc * r[:, None] + b
        by.append(np.abs(a) * r[:, None] * (d_xc + np.abs(xc) * (d_rr[:, None] + 3.0 * U)) + U * np.abs(y))
        bm.append(d_mean)
        bs.append(d_sd)
    return np.concatenate(by), np.concatenate(bm), np.concatenate(bs)


def backward_bound(dy, x, a, eps=EPS, dres=None, D=None, e=None):
    """Bound of dx (rows, d), and of the da / db column sums their two ingredients each: (sum_rows d_t, sum_rows |t|) as
    (da_err, da_abs, db_err, db_abs), for colsum_bound.  e: the error dy already carries, per entry (None: 0)."""
    dy, x, a = _f64(dy), _f64(x), _f64(a)
    n = x.shape[-1]
    D = depth(n) if D is None else D
    bdx = []
    acc = [np.zeros(n) for _ in range(4)]
    for s in range(0, x.shape[0], CHUNK):
        xc, sd, r, d_mean, d_xc, d_sd, d_rr = _stats_model(x[s:s + CHUNK], eps, D)
        dyc = dy[s:s + CHUNK]
        ec = np.zeros_like(dyc) if e is None else _f64(e)[s:s + CHUNK]
        rc, d_rc = r[:, None], d_rr[:, None]
        g = dyc * a
        d_g = U * np.abs(g) + np.abs(a) * ec
        sg = g.sum(-1)
        mg = sg / n
        d_mg = (d_g.sum(-1) + D * U * np.abs(g).sum(-1)) / n + U * np.abs(mg)
        t = g * xc
        sgx = t.sum(-1)
        d_sgx = (np.abs(g) * d_xc + np.abs(xc) * d_g + U * np.abs(t)).sum(-1) + D * U * np.abs(t).sum(-1)
        coef = r * r * sgx / ((n - 1) * sd)
        d_coef = np.abs(coef) * (2.0 * d_rr + d_sd / sd + 4.0 * U) + r * r * d_sgx / ((n - 1) * sd)
        t1 = rc * (g - mg[:, None])
        t2 = coef[:, None] * xc
        dx = t1 - t2
        b = (rc * (d_g + d_mg[:, None] + U * np.abs(g - mg[:, None])) + np.abs(t1) * (d_rc + U)
             + np.abs(coef)[:, None] * d_xc + np.abs(xc) * d_coef[:, None] + U * np.abs(t2) + 2.0 * U * np.abs(dx))
        if dres is not None:
            b = b + U * np.abs(dx + _f64(dres)[s:s + CHUNK])
        bdx.append(b)
        ta = dyc * xc * rc
        acc[0] += (np.abs(dyc) * rc * d_xc + np.abs(ta) * (d_rc + 2.0 * U) + ec * np.abs(xc) * rc).sum(0)
        acc[1] += np.abs(ta).sum(0)
        acc[2] += ec.sum(0)
        acc[3] += np.abs(dyc).sum(0)
    return (np.concatenate(bdx),) + tuple(acc)


def colsum_bound(err, tabs, levels, nblocks, c):
    """Bound of a da / db column sum: err = sum_rows d_t, tabs = sum_rows |t|, levels = the chain and tree inside a block,
    c = what the output held before the call."""
    return err + (levels + nblocks) * U * tabs + nblocks * U * np.abs(_f64(c))


def ratio(err, bound):
    """Largest error / bound; an entry whose bound is 0 must be exact."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.isfinite(err).all() and np.isfinite(bound).all()
    zero = bound == 0
    assert (err[zero] == 0).all()
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
