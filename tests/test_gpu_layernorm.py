"""Every LayerNorm kernel on a real MI355X against the float64 reference and the fp32 error model of tests/ln_ref.py (read its
docstring first: formulas, bounds, input classes): the ten standalone instances of csrc/ortk_norm.hip, every row edge of the backward's
row pipeline and both block heights, every argument form, and the two ln_mode epilogues of ortk_gemm with all four short-panel
instances.  tests/test_ln_ref_host.py shows on the CPU that the asserted 4 bounds are sound and sharp.

Every buffer a kernel reads or writes is a slice of a NaN-filled allocation with 64 elements of NaN on both sides (_fenced); the
fences are asserted intact after every call, outputs are asserted finite (a read past an input reaches a sum as NaN).  References are
float64 on the CPU, from x itself; the backward's statistics are the kernel's own forward's.  Row i of every input is of class
i mod 5 (backward) or i mod 6 (forward, with the constant rows) of ln_ref.class_rows.  Each test prints the largest error / bound it
saw (profiles/layernorm_operator_tests.txt).

No constant row enters a backward case: the reference's own backward is 0 / 0 there (the gradient of std at zero variance)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ln_ref as R

pytestmark = pytest.mark.gpu

EINVAL = -1
U, MARGIN, EPS = R.U, R.MARGIN, R.EPS
PAD = 64                     # elements of NaN around every slice (a multiple of 8: 16 bytes in both element types)
TDT = {0: torch.float32, 1: torch.bfloat16}


@pytest.fixture(scope="module")
def L():
    import sparse_image_captioning_amd as P
    P._lib.require_gpu()
    return P._lib


# ------------------------------------------------------------------------------------------------ fenced buffers
class Fenced:
    """One NaN-filled device buffer holding `parts` (CPU tensors of one float type) as slices that start on 16-byte boundaries
    (+ `shift` elements), PAD elements of NaN between and around them."""

    def __init__(self, parts, dtype=torch.float32, shift=0):
        self.spans, off = [], PAD
        for p in parts:
            off = -(-off // 8) * 8 + shift
            self.spans.append((off, p.numel()))
            off += p.numel() + PAD
        host = torch.full((off,), float("nan"), dtype=dtype)
        for (o, n), p in zip(self.spans, parts):
            host[o:o + n] = p.reshape(-1).to(dtype)
        self.buf = host.cuda()
        self.views = [self.buf[o:o + n] for o, n in self.spans]
        for v in self.views:
            assert v.data_ptr() % 16 == (shift * v.element_size()) % 16

    def intact(self):
        nan = torch.isnan(self.buf)
        for o, n in self.spans:
            nan[o:o + n] = True
        return bool(nan.all())


def _nan(n):
    return torch.full((n,), float("nan"))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y))


def _np64(t):
    return t.detach().cpu().double().numpy()


# ------------------------------------------------------------------------------------------------ the standalone forward
#                     scalar, NREG 8                                  vector, NREG 8       scalar, NREG 32                    vector, NREG 32                  grid tail
FWD_CASES = [(1, 2), (5, 3), (7, 63), (9, 65), (6, 510), (3, 508), (4, 512), (5, 513), (3, 1030), (3, 2047), (2, 516), (2, 2044), (5, 2048), (1027, 8)]


def _params(d, seed):
    g = np.random.default_rng(seed)
    return (1 + 0.1 * g.standard_normal(d)).astype(np.float32), (0.1 * g.standard_normal(d)).astype(np.float32)


def _run_fwd(L, x, a, b, y_dtype=0, stats=True, shift=0):
    """One ortk_layernorm_fwd into fresh fenced buffers; returns (y, stats or None) on the CPU."""
    rows, d = x.shape
    fx, fp = Fenced([_t(x)], shift=shift), Fenced([_t(a), _t(b)])
    fy, fs = Fenced([_nan(rows * d)], TDT[y_dtype]), Fenced([_nan(rows * 2)])
    L.check(L.lib().ortk_layernorm_fwd(L.ptr(fx.views[0]), L.ptr(fp.views[0]), L.ptr(fp.views[1]), L.ptr(fy.views[0]), y_dtype,
                                       L.ptr(fs.views[0]) if stats else None, rows, d, EPS, L.stream_ptr()), "ortk_layernorm_fwd")
    torch.cuda.synchronize()
    assert fy.intact() and fs.intact() and fx.intact() and fp.intact(), "the forward wrote outside an output"
    y, st = fy.views[0].cpu().reshape(rows, d), fs.views[0].cpu().reshape(rows, 2)
    assert torch.isfinite(y.float()).all(), "a NaN in y: not every entry written, or something read past an input"
    if stats:
        assert torch.isfinite(st).all()
    else:
        assert torch.isnan(st).all(), "stats = NULL, and the statistics were written somewhere"
    return y, (st if stats else None)


def _check_fwd(tag, x, kind, a, b, y, st, margin=MARGIN):
    ry, rm, rs = R.forward(x, a, b)
    by, bm, bs = R.forward_bound(x, a, b)
    r = (R.ratio(np.abs(_np64(y) - ry), by), R.ratio(np.abs(_np64(st[:, 0]) - rm), bm), R.ratio(np.abs(_np64(st[:, 1]) - rs), bs))
    print(f"ln {tag}: y error / bound {r[0]:.4f}, mean {r[1]:.4f}, sd {r[2]:.4f}")
    assert max(r) <= margin
    const = _t(kind == 5)
    if const.any():      # class 5: exact
        assert (y[const] == _t(b)).all() and (st[const][:, 0] == 1.5).all() and (st[const][:, 1] == 0.0).all()
    return by


@pytest.mark.parametrize("rows,d", FWD_CASES)
def test_forward(L, rows, d):
    """y and the statistics of every forward instance against the model; then the exact relations: a rerun gives the same bits,
    stats = NULL the same y, y_dtype = 1 the bf16 rounding of the fp32 y."""
    x, kind = R.class_rows(rows, d, 10 * rows + d, R.FWD_CLASSES)
    a, b = _params(d, d)
    y, st = _run_fwd(L, x, a, b)
    _check_fwd(f"fwd rows={rows} d={d}", x, kind, a, b, y, st)
    y2, st2 = _run_fwd(L, x, a, b)
    assert _same(y, y2) and _same(st, st2), "a rerun changed bits"
    y3, _ = _run_fwd(L, x, a, b, stats=False)
    assert _same(y, y3), "stats = NULL changed y"
    y16, st16 = _run_fwd(L, x, a, b, y_dtype=1)
    assert _same(y16, y.bfloat16()) and _same(st16, st), "the bf16 y is not the rounding of the fp32 y"


@pytest.mark.parametrize("d", [3, 512, 516, 1030])
def test_forward_constant_rows(L, d):
    """Rows of the constant 1.5 through every forward instance: y == b, sd == 0, mean == 1.5, exactly."""
    x = np.full((5, d), 1.5, np.float32)
    a, b = _params(d, d + 1)
    y, st = _run_fwd(L, x, a, b)
    assert (y == _t(b)).all() and (st[:, 0] == 1.5).all() and (st[:, 1] == 0.0).all()


def test_forward_misaligned_rows_take_the_scalar_form(L):
    """(4, 512) with x one float past a 16-byte boundary: the scalar instance, within 4 bounds of the reference and 2 of the
    aligned run."""
    rows, d = 4, 512
    x, kind = R.class_rows(rows, d, 10 * rows + d, R.FWD_CLASSES)
    a, b = _params(d, d)
    y0, st0 = _run_fwd(L, x, a, b)
    y1, st1 = _run_fwd(L, x, a, b, shift=1)
    by = _check_fwd("fwd rows=4 d=512 misaligned", x, kind, a, b, y1, st1)
    r = R.ratio(np.abs(_np64(y1) - _np64(y0)), by)
    print(f"ln fwd rows=4 d=512 misaligned vs aligned: y difference / bound {r:.4f}")
    assert r <= 2.0


def test_forward_refusals(L):
    """d = 1, d = 2049, y_dtype = 2 and a NULL pointer return -1; rows = 0 returns 0; none of them writes anything."""
    lib, st = L.lib(), L.stream_ptr()
    fx, fp = Fenced([torch.ones(4 * 2049)]), Fenced([torch.ones(2049), torch.ones(2049)])
    fy, fs = Fenced([_nan(4 * 2049)]), Fenced([_nan(8)])
    x, a, b, y, s = L.ptr(fx.views[0]), L.ptr(fp.views[0]), L.ptr(fp.views[1]), L.ptr(fy.views[0]), L.ptr(fs.views[0])
    assert lib.ortk_layernorm_fwd(x, a, b, y, 0, s, 4, 1, EPS, st) == EINVAL
    assert lib.ortk_layernorm_fwd(x, a, b, y, 0, s, 4, 2049, EPS, st) == EINVAL
    assert lib.ortk_layernorm_fwd(x, a, b, y, 2, s, 4, 8, EPS, st) == EINVAL
    for args in ((None, a, b, y), (x, None, b, y), (x, a, None, y), (x, a, b, None)):
        assert lib.ortk_layernorm_fwd(*args, 0, s, 4, 8, EPS, st) == EINVAL
    assert lib.ortk_layernorm_fwd(x, a, b, y, 0, s, 0, 8, EPS, st) == 0
    torch.cuda.synchronize()
    assert torch.isnan(fy.buf).all() and torch.isnan(fs.buf).all()


# ------------------------------------------------------------------------------------------------ the standalone backward
#        dres   dz (None | 0 fp32 | 1 bf16)   p    drop_rows
OPTIONS = {
    "A": (True, 1, 0.1, False),
    "B": (False, 0, 0.1, True),
    "C": (True, None, 0.0, False),
    "D": (False, 1, 0.0, False),
}
DROP_SEED = 1234
_CASES = {}


def _bwd_case(L, rows, d, bf16_dy=False):
    """Inputs, the kernel's own forward statistics and the float64 reference (without dres) of one backward case; computed once."""
    key = (rows, d, bf16_dy)
    if key not in _CASES:
        x, kind = R.class_rows(rows, d, 7 * rows + d, R.BWD_CLASSES)
        g = np.random.default_rng(rows + 13 * d)
        a, b = _params(d, d + 2)
        dy = _t(g.standard_normal((rows, d)).astype(np.float32))
        if bf16_dy:
            dy = dy.bfloat16()
        dres = g.standard_normal((rows, d)).astype(np.float32)
        ca, cb = g.standard_normal(d).astype(np.float32), g.standard_normal(d).astype(np.float32)
        tall = 2 * rows + 5
        perm = np.random.default_rng(rows).permutation(tall)[:rows].astype(np.int32)
        _, st = _run_fwd(L, x, a, b)
        dyf = dy.float().numpy()
        dx, da, db = R.backward(dyf, x, a)
        bdx, ea, ta, eb, tb = R.backward_bound(dyf, x, a)
        lv, nb = R.colsum_shape(rows)
        _CASES[key] = dict(rows=rows, d=d, x=x, a=a, dy=dy, dres=dres, ca=ca, cb=cb, perm=perm, st=st, dx=dx, da=da, db=db, bdx=bdx,
                           ba=R.colsum_bound(ea, ta, lv, nb, ca), bb=R.colsum_bound(eb, tb, lv, nb, cb), ta=ta, tb=tb, nb=nb)
    return _CASES[key]


def _run_bwd(L, c, opt, shift=0):
    """One ortk_layernorm_bwd_dt into fresh fenced buffers with the options `opt`; returns dx, da, db, dz on the CPU."""
    with_res, dz_dt, p, keyed = OPTIONS[opt]
    rows, d = c["rows"], c["d"]
    bf = c["dy"].dtype == torch.bfloat16
    fx, fdy = Fenced([_t(c["x"])], shift=shift), Fenced([c["dy"]], c["dy"].dtype)
    fin = Fenced([_t(c["a"]), c["st"], _t(c["dres"])])
    fdx, fg = Fenced([_nan(rows * d)]), Fenced([_t(c["ca"]), _t(c["cb"])])
    fdz = Fenced([_nan(rows * d)], TDT[dz_dt or 0])
    rows_d = _t(c["perm"]).cuda() if keyed else None
    L.check(L.lib().ortk_layernorm_bwd_dt(L.ptr(fdy.views[0]), int(bf), L.ptr(fx.views[0]), L.ptr(fin.views[0]), L.ptr(fin.views[1]),
                                          L.ptr(fin.views[2]) if with_res else None, L.ptr(fdx.views[0]), L.ptr(fg.views[0]), L.ptr(fg.views[1]),
                                          rows, d, EPS, L.ptr(fdz.views[0]) if dz_dt is not None else None, dz_dt or 0, p, DROP_SEED,
                                          L.ptr(rows_d), L.stream_ptr()), "ortk_layernorm_bwd_dt")
    torch.cuda.synchronize()
    assert all(f.intact() for f in (fx, fdy, fin, fdx, fg, fdz)), "the backward wrote outside an output"
    dx, dz = fdx.views[0].cpu().reshape(rows, d), fdz.views[0].cpu().reshape(rows, d)
    da, db = fg.views[0].cpu(), fg.views[1].cpu()
    assert torch.isfinite(dx).all() and torch.isfinite(da).all() and torch.isfinite(db).all(), "a NaN: an entry not written, or a read past an input"
    # the exact relations of dz: what ortk_dropout_apply(_rows) writes from the kernel's own dx; p = 0: dx rounded
    if dz_dt is None:
        assert torch.isnan(dz.float()).all(), "dz = NULL, and something was written"
        dz = None
    else:
        z = torch.full((rows, d), float("nan"), dtype=TDT[dz_dt], device="cuda")
        dxd = fdx.views[0]
        if keyed:
            L.check(L.lib().ortk_dropout_apply_rows(L.ptr(dxd), L.ptr(z), dz_dt, rows, d, p, DROP_SEED, L.ptr(rows_d), L.stream_ptr()), "ortk_dropout_apply_rows")
        else:
            L.check(L.lib().ortk_dropout_apply(L.ptr(dxd), L.ptr(z), dz_dt, rows * d, p, DROP_SEED, L.stream_ptr()), "ortk_dropout_apply")
        torch.cuda.synchronize()
        assert _same(dz, z.cpu()), "dz is not the dropout of the kernel's own dx"
        if p == 0.0:
            assert _same(dz, dx.to(TDT[dz_dt])), "p = 0: dz is not dx rounded"
    return dx, da, db, dz


def _check_bwd(tag, c, opt, out, margin=MARGIN):
    with_res = OPTIONS[opt][0]
    dx, da, db, _ = out
    ref, bdx = c["dx"], c["bdx"]
    if with_res:
        ref = ref + c["dres"]
        bdx = bdx + U * np.abs(ref)
    r = (R.ratio(np.abs(_np64(dx) - ref), bdx), R.ratio(np.abs(_np64(da) - (c["ca"] + c["da"])), c["ba"]),
         R.ratio(np.abs(_np64(db) - (c["cb"] + c["db"])), c["bb"]))
    print(f"ln {tag} options {opt}: dx error / bound {r[0]:.4f}, da {r[1]:.4f}, db {r[2]:.4f}")
    assert max(r) <= margin
    return bdx


def _check_rerun(tag, c, opt, out, out2):
    """dx and dz bit-identical; da / db, whose block sums arrive by float atomics in any order, within 2 nblocks u sum|term|."""
    assert _same(out[0], out2[0]) and (out[3] is None or _same(out[3], out2[3])), "a rerun changed bits of dx / dz"
    ra = R.ratio(np.abs(_np64(out[1]) - _np64(out2[1])), 2 * c["nb"] * U * c["ta"])
    rb = R.ratio(np.abs(_np64(out[2]) - _np64(out2[2])), 2 * c["nb"] * U * c["tb"])
    print(f"ln {tag} options {opt}: rerun da difference / bound {ra:.4f}, db {rb:.4f}")
    assert ra <= 1.0 and rb <= 1.0


def _all_options(L, tag, c, options="ABCD", rerun=True):
    for opt in options:
        out = _run_bwd(L, c, opt)
        _check_bwd(tag, c, opt, out)
        if rerun:
            _check_rerun(tag, c, opt, out, _run_bwd(L, c, opt))


@pytest.mark.parametrize("d", [2, 3, 8, 100, 510, 516, 1030, 2044, 2047, 2048])
def test_backward_instances(L, d):
    """The four generic instances at rows = 37 (a full block of 32 and a block whose waves hold 2, 1, 1, 1 rows), each under the four
    option sets: with and without dres, dz absent / fp32 / bf16, p = 0 and 0.1, draws keyed by a row map."""
    _all_options(L, f"bwd rows=37 d={d}", _bwd_case(L, 37, d))


@pytest.mark.parametrize("form", ["eight_f32", "eight_bf16", "four"])
def test_backward_width_512_forms(L, form):
    """d = 512 in its three forms: ln_bwd512_kernel<float>, ln_bwd512_kernel<__bf16> (bf16 dy), and the four-column generic instance
    (ortk_tuning.ln_fuse bit 2)."""
    c = _bwd_case(L, 37, 512, bf16_dy=form == "eight_bf16")
    prev = L.set_tuning(ln_fuse=4 if form == "four" else 0)
    try:
        _all_options(L, f"bwd rows=37 d=512 {form}", c)
    finally:
        L.set_tuning(**prev)


@pytest.mark.parametrize("d", [8, 6])
@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65])
def test_backward_row_edges(L, rows, d):
    """The row pipeline (fetch(row + 4), rr + 4 < rows_per_block) at every count around a wave round and a block, vector and scalar."""
    _all_options(L, f"bwd rows={rows} d={d}", _bwd_case(L, rows, d), "AB")


@pytest.mark.parametrize("bf16_dy", [False, True])
@pytest.mark.parametrize("rows", [1, 3, 5, 33])
def test_backward_row_edges_width_512(L, rows, bf16_dy):
    _all_options(L, f"bwd rows={rows} d=512 {'bf16' if bf16_dy else 'f32'} dy", _bwd_case(L, rows, 512, bf16_dy), "AB")


@pytest.mark.parametrize("rows", [16383, 16384, 16387])
def test_backward_block_height_switch(L, rows):
    """32 rows per block below 16 384 rows, 64 from there on (257 blocks at 16 387, the last of three rows): one launch each."""
    c = _bwd_case(L, rows, 8)
    assert R.colsum_shape(rows) == ((10, 512) if rows < 16384 else (18, -(-rows // 64)))
    _check_bwd(f"bwd rows={rows} d=8", c, "A", _run_bwd(L, c, "A"))


def test_backward_executor_call_at_the_tall_height(L):
    """The executor's own call: 16 387 rows of width 512, bf16 dy, bf16 dz, p = 0.1, residual gradient; one launch."""
    c = _bwd_case(L, 16387, 512, bf16_dy=True)
    _check_bwd("bwd rows=16387 d=512 bf16 dy", c, "A", _run_bwd(L, c, "A"))


def test_backward_misaligned_rows_at_width_512(L):
    """x one float past a 16-byte boundary at d = 512: the generic scalar instance, within 4 bounds of the reference and 2 of the
    aligned (eight-column) result; a bf16 dy with misaligned rows, or at another width, is refused."""
    c = _bwd_case(L, 37, 512)
    out0 = _run_bwd(L, c, "A")
    out1 = _run_bwd(L, c, "A", shift=1)
    bdx = _check_bwd("bwd rows=37 d=512 misaligned", c, "A", out1)
    r = (R.ratio(np.abs(_np64(out1[0]) - _np64(out0[0])), bdx), R.ratio(np.abs(_np64(out1[1]) - _np64(out0[1])), c["ba"]),
         R.ratio(np.abs(_np64(out1[2]) - _np64(out0[2])), c["bb"]))
    print(f"ln bwd rows=37 d=512 misaligned vs aligned: dx difference / bound {r[0]:.4f}, da {r[1]:.4f}, db {r[2]:.4f}")
    assert max(r) <= 2.0
    c16 = _bwd_case(L, 37, 512, bf16_dy=True)
    with pytest.raises(L.OrtkError):
        _run_bwd(L, c16, "A", shift=1)
    c100 = dict(_bwd_case(L, 37, 100))
    c100["dy"] = c100["dy"].bfloat16()
    with pytest.raises(L.OrtkError):
        _run_bwd(L, c100, "A")


def test_backward_refusals(L):
    """dz_dtype = 2, drop_p = 1 and drop_p < 0 return -1 and write nothing."""
    lib, st = L.lib(), L.stream_ptr()
    rows, d = 5, 8
    fin = Fenced([torch.ones(rows * d), torch.ones(rows * d), torch.ones(d), torch.ones(rows * 2)])
    fo = Fenced([_nan(rows * d), _nan(rows * d), _nan(d), _nan(d)])
    dy, x, a, s = (L.ptr(v) for v in fin.views)
    dx, dz, da, db = (L.ptr(v) for v in fo.views)
    call = lambda dzt, p: lib.ortk_layernorm_bwd_drop(dy, x, a, s, None, dx, da, db, rows, d, EPS, dz, dzt, p, 1, st)
    assert call(2, 0.1) == EINVAL and call(0, 1.0) == EINVAL and call(1, -0.1) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(fo.buf).all()


# ------------------------------------------------------------------------------------------------ the fused epilogues of ortk_gemm
GK = 64


def _gemm_args(L, A, W, Cout, M, **kw):
    a = L.GemmArgs()
    a.A, a.B, a.C = A.data_ptr(), W.data_ptr(), Cout.data_ptr()
    a.lda, a.ldb, a.ldc = GK, GK, 512
    a.M, a.N, a.K, a.precision, a.a_dtype, a.b_dtype = M, 512, GK, 1, 1, 1
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            setattr(a, k, v.data_ptr())
            if k == "resid":
                a.ldr = 512
        else:
            setattr(a, k, v)
    return a


def _operands(M, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, GK, generator=g).bfloat16()
    W = (torch.randn(512, GK, generator=g) * GK ** -0.5).bfloat16()
    prod = A.double().numpy() @ W.double().numpy().T
    e = (GK + 2) * U * (A.double().abs().numpy() @ W.double().abs().numpy().T)
    return A, W, prod, e


def _keep_scale(L, n, p, seed):
    """keep / (1 - p) per element as the kernels draw it (element index row * N + column), in the kernels' own fp32 scale."""
    ones, out = torch.ones(n, device="cuda"), torch.empty(n, device="cuda")
    L.check(L.lib().ortk_dropout_apply(L.ptr(ones), L.ptr(out), 0, n, p, seed, L.stream_ptr()), "ortk_dropout_apply")
    return _np64(out)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("M", [1, 127, 129])
def test_gemm_fused_layernorm_forward(L, M, p):
    """ortk_gemm(ln_mode = 1) on gemm_bf16_row512_kernel (asserted through ortk_gemm_plan).  C against the float64 product of the
    bf16 operands + bias, the dropout draws, + residual, at (K + 2) u sum|a||w| / (1 - p) + u |C|; ln_y and ln_stats against
    forward() of the kernel's own C under the forward model with the kernel's D; the bf16 ln_y is the rounding of the fp32 one."""
    A, W, prod, e = _operands(M, 100 + M)
    res, kind = R.class_rows(M, 512, 200 + M, R.BWD_CLASSES)
    ga, gb = _params(512, 5)
    bias = np.random.default_rng(M).standard_normal(512).astype(np.float32)
    fa, fw = Fenced([A], torch.bfloat16), Fenced([W], torch.bfloat16)
    fin = Fenced([_t(bias), _t(res), _t(ga), _t(gb)])
    outs = {}
    for ydt in (0, 1):
        fc, fy, fs = Fenced([_nan(M * 512)]), Fenced([_nan(M * 512)], TDT[ydt]), Fenced([_nan(M * 2)])
        args = _gemm_args(L, fa.views[0], fw.views[0], fc.views[0], M, bias=fin.views[0], resid=fin.views[1], ln_mode=1, ln_y_dtype=ydt,
                          ln_a=fin.views[2], ln_b=fin.views[3], ln_y=fy.views[0], ln_stats=fs.views[0], ln_eps=EPS, drop_p=p, drop_seed=77)
        assert L.gemm_plan(args) == ["bf16_row512"]
        L.check(L.lib().ortk_gemm(C.byref(args), L.stream_ptr()), "ortk_gemm")
        torch.cuda.synchronize()
        assert all(f.intact() for f in (fa, fw, fin, fc, fy, fs)), "the fused forward wrote outside an output"
        outs[ydt] = (fc.views[0].cpu().reshape(M, 512), fy.views[0].cpu().reshape(M, 512), fs.views[0].cpu().reshape(M, 2))
        assert all(torch.isfinite(t.float()).all() for t in outs[ydt])
    c, y, st = outs[0]
    scale = _keep_scale(L, M * 512, p, 77).reshape(M, 512) if p > 0 else np.ones((M, 512))
    ik = scale.max()
    ref = (prod + bias) * scale + res
    rc = R.ratio(np.abs(_np64(c) - ref), ik * e + U * np.abs(ref))
    ck = _np64(c)
    ry, rm, rs = R.forward(ck, ga, gb)
    by, bm, bs = R.forward_bound(ck, ga, gb, D=R.D_ROW512)
    r = (R.ratio(np.abs(_np64(y) - ry), by), R.ratio(np.abs(_np64(st[:, 0]) - rm), bm), R.ratio(np.abs(_np64(st[:, 1]) - rs), bs))
    print(f"ln gemm ln_mode=1 M={M} p={p}: C error / bound {rc:.4f}, ln_y {r[0]:.4f}, mean {r[1]:.4f}, sd {r[2]:.4f}")
    assert rc <= MARGIN and max(r) <= MARGIN
    if p > 0:
        assert 0.0 < (scale == 0).mean() < 0.25
    assert _same(outs[1][0], c) and _same(outs[1][2], st) and _same(outs[1][1], y.bfloat16())


_GEMM_BWD = {}


def _gemm_bwd_case(L, M):
    if M not in _GEMM_BWD:
        A, W, prod, e = _operands(M, 300 + M)
        x, kind = R.class_rows(M, 512, 400 + M, R.BWD_CLASSES)
        ga, gb = _params(512, 9)
        g = np.random.default_rng(M + 1)
        dres = g.standard_normal((M, 512)).astype(np.float32)
        ca, cb = g.standard_normal(512).astype(np.float32), g.standard_normal(512).astype(np.float32)
        _, st = _run_fwd(L, x, ga, gb)
        mt = min(5, max(2, -(-M // 4096)))
        nb = -(-M // (16 * mt))
        dx, da, db = R.backward(prod, x, ga)
        bdx, ea, ta, eb, tb = R.backward_bound(prod, x, ga, D=R.D_ROWLN_BWD, e=e)
        _GEMM_BWD[M] = dict(A=A, W=W, x=x, ga=ga, dres=dres, ca=ca, cb=cb, st=st, mt=mt, dx=dx, da=da, db=db, bdx=bdx,
                            ba=R.colsum_bound(ea, ta, mt + 4, nb, ca), bb=R.colsum_bound(eb, tb, mt + 4, nb, cb))
    return _GEMM_BWD[M]


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("M", [1, 31, 33, 8193, 12289, 16385])
def test_gemm_fused_layernorm_backward(L, M, with_res):
    """ortk_gemm(ln_mode = 2) on gemm_bf16_rowln_bwd_kernel<MT>, MT = 2 (M <= 8 192), 3, 4, 5 (asserted through ortk_gemm_plan).  dy
    is the float64 product of the bf16 operands; the product's (K + 2) u sum|a||w| enters the backward model as the error of dy.
    C, ln_da, ln_db against backward() of x; ln_y is what ortk_dropout_apply writes from the kernel's own C, bit for bit."""
    c = _gemm_bwd_case(L, M)
    p, seed = 0.1, 99
    fa, fw = Fenced([c["A"]], torch.bfloat16), Fenced([c["W"]], torch.bfloat16)
    fin = Fenced([_t(c["x"]), _t(c["ga"]), c["st"], _t(c["dres"])])
    fc, fz, fg = Fenced([_nan(M * 512)]), Fenced([_nan(M * 512)], torch.bfloat16), Fenced([_t(c["ca"]), _t(c["cb"])])
    kw = dict(ln_dres=fin.views[3]) if with_res else {}
    args = _gemm_args(L, fa.views[0], fw.views[0], fc.views[0], M, ln_mode=2, ln_y_dtype=1, ln_x=fin.views[0], ln_a=fin.views[1],
                      ln_stats=fin.views[2], ln_y=fz.views[0], ln_da=fg.views[0], ln_db=fg.views[1], ln_eps=EPS, drop_p=p, drop_seed=seed, **kw)
    assert L.gemm_plan(args) == [f"bf16_rowln_bwd<{c['mt']}>"]
    L.check(L.lib().ortk_gemm(C.byref(args), L.stream_ptr()), "ortk_gemm")
    torch.cuda.synchronize()
    assert all(f.intact() for f in (fa, fw, fin, fc, fz, fg)), "the fused backward wrote outside an output"
    dx, dz = fc.views[0].cpu().reshape(M, 512), fz.views[0].cpu().reshape(M, 512)
    da, db = fg.views[0].cpu(), fg.views[1].cpu()
    assert torch.isfinite(dx).all() and torch.isfinite(da).all() and torch.isfinite(db).all()
    ref, bdx = c["dx"], c["bdx"]
    if with_res:
        ref = ref + c["dres"]
        bdx = bdx + U * np.abs(ref)
    r = (R.ratio(np.abs(_np64(dx) - ref), bdx), R.ratio(np.abs(_np64(da) - (c["ca"] + c["da"])), c["ba"]),
         R.ratio(np.abs(_np64(db) - (c["cb"] + c["db"])), c["bb"]))
    print(f"ln gemm ln_mode=2 M={M} MT={c['mt']} dres={int(with_res)}: C error / bound {r[0]:.4f}, ln_da {r[1]:.4f}, ln_db {r[2]:.4f}")
    assert max(r) <= MARGIN
    z = torch.full((M, 512), float("nan"), dtype=torch.bfloat16, device="cuda")
    L.check(L.lib().ortk_dropout_apply(L.ptr(fc.views[0]), L.ptr(z), 1, M * 512, p, seed, L.stream_ptr()), "ortk_dropout_apply")
    torch.cuda.synchronize()
    assert _same(dz, z.cpu()), "ln_y is not the dropout of the kernel's own C"
