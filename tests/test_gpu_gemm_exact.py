"""ortk_gemm / ortk_wgrad_group on exact operands (tests/gemm_exact.py): integer-valued matrices whose products and partial sums stay
below 2^24, so that fp32 accumulation is exact whatever its order and the result must equal a float64 reference of the whole epilogue BIT
FOR BIT — through every kernel instance the dispatch plan can launch (ortk_gemm_plan says which one a case runs, and the case asserts it
is the one it was built for).  Operands sit with padded leading dimensions inside NaN-filled buffers (a read outside the operand
poisons the result), C inside a sentinel (a write outside (M, N) shows)."""
import ctypes as C
import os
import time

import pytest
import torch

import gemm_exact as X
from exact_gpu import SLACK, _KEEP, mismatch, place

pytestmark = pytest.mark.gpu

_PLANS = {}
_RECORD = []
_REF = {}


@pytest.fixture(scope="module")
def L():
    import sparse_image_captioning_amd as P
    P._lib.require_gpu()
    return P._lib


@pytest.fixture(autouse=True)
def release_buffers():
    """Whatever a case placed on the device goes when the case ends, passed or failed."""
    yield
    del _KEEP[:]


def keep_mask(L, c, o, seed):
    """0 / 2 per output element: the draws of ortk_dropout_apply on ones over the index space, taken at each element's index"""
    idx = X.drop_index(c, o)
    n = int(idx.max()) + 1
    ones, out = torch.ones(n, device="cuda"), torch.empty(n, device="cuda")
    L.check(L.lib().ortk_dropout_apply(L.ptr(ones), L.ptr(out), 0, n, X.DROP_P, seed, L.stream_ptr()), "ortk_dropout_apply")
    torch.cuda.synchronize()
    k = out[idx.cuda()].cpu().double()
    assert set(k.unique().tolist()) <= {0.0, 2.0}
    return k


def run_case(L, c):
    o = X.operands(c)
    lda, ldb, ldc = X.lds(c)
    dt = lambda d: torch.bfloat16 if d else torch.float32
    A = o["A"].t().contiguous() if c.ta else o["A"]
    B = o["B"].t().contiguous() if c.tb else o["B"]
    ptr, have = {}, []
    _, _, ptr["A"] = place(A, lda, c.off[0], dt(c.adt))
    _, _, ptr["B"] = place(B, ldb, c.off[1], dt(c.bdt))
    eo = c.off[2]          # the epilogue's operands are as aligned as C is
    for k, ld, d in (("bias", None, 0), ("rowscale", None, 0), ("resid", ldc, 0), ("gate", ldc, int(c.gate == "bf16"))):
        if k in o:
            _, _, ptr[k] = place(o[k], ld, eo, dt(d))
            have.append(k)
    if "rows" in o:
        _, _, ptr["rows"] = place(o["rows"], None, 0, torch.int32, fill=0)
    if c.ln:
        for k, t in (("ln_a", torch.ones(c.N)), ("ln_b", torch.zeros(c.N)), ("ln_stats", torch.zeros(c.M, 2))):
            _, _, ptr[k] = place(t, None, 0, torch.float32)
        _, _, ptr["ln_y"] = place(torch.zeros(c.M, c.N), None, 0, torch.bfloat16)
    seed = 1000 + c.seed % 1000
    keep = keep_mask(L, c, o, seed) if c.drop else None
    want, want_cs = X.expected(c, o, keep)
    want32 = want.float()
    assert torch.equal(want32.double(), want)                      # (the reference itself is an exact fp32 value)
    want_dev = (want32.bfloat16() if c.cdt else want32).cuda()     # a bf16 C: the exact fp32 result, rounded by torch

    def launch():
        c0 = o["C0"] if c.accumulate else torch.full((c.M, c.N), X.SENTINEL, dtype=torch.float64)
        cbuf, cview, ptr["C"] = place(c0, ldc, c.off[2], dt(c.cdt), fill=X.SENTINEL)
        csbuf = csview = None
        if c.colsum:
            csbuf, csview, ptr["colsum"] = place(o["cs0"], None, 0, torch.float32, fill=X.SENTINEL)
        a = X.fill_args(c, L.GemmArgs(), ptr, have + (["colsum"] if c.colsum else []))
        assert a.drop_seed == (seed if c.drop else 0)
        plan = L.gemm_plan(a)
        assert plan == c.plan, (c.name, plan)
        L.check(L.lib().ortk_gemm(C.byref(a), L.stream_ptr()), "ortk_gemm")
        torch.cuda.synchronize()
        return plan, cbuf, cview, csbuf, csview

    prev = L.set_tuning(**c.tuning)
    try:
        plan, cbuf, cview, csbuf, csview = launch()
        again = None if c.accumulate else launch()
    finally:
        L.set_tuning(**prev)
    _PLANS[c.name] = plan
    assert torch.equal(cview, want_dev), mismatch(cview.cpu(), want_dev.cpu(), c.name)
    rest = cbuf.clone()
    rest[SLACK + c.off[2]: SLACK + c.off[2] + c.M * ldc].view(c.M, ldc)[:, :c.N] = X.SENTINEL
    assert bool((rest == X.SENTINEL).all()), "%s: written outside (M, N): %d elements" % (c.name, int((rest != X.SENTINEL).sum()))
    if c.colsum:
        assert torch.equal(csview[0].cpu().double(), want_cs), mismatch(csview[0].cpu().double(), want_cs, c.name + " colsum")
        rest = csbuf.clone(); rest[SLACK: SLACK + c.M] = X.SENTINEL
        assert bool((rest == X.SENTINEL).all()), c.name + ": column sums written outside M"
    if again is not None:      # same bytes on a rerun, column sums and the surroundings of C included
        assert torch.equal(again[1].view(torch.int16 if c.cdt else torch.int32), cbuf.view(torch.int16 if c.cdt else torch.int32)), c.name + ": rerun differs"
        if c.colsum:
            assert torch.equal(again[3], csbuf)
    return plan


@pytest.mark.parametrize("c", X.CASES, ids=lambda c: c.name)
def test_gemm_exact(L, c):
    t0, plan, result = time.perf_counter(), c.plan, "FAIL"
    try:
        plan = run_case(L, c)
        result = "pass"
    finally:          # (a failing case leaves its line too, with the plan it was built for)
        _RECORD.append("%-34s %5d x %5d x %4d %s prec %d %-10s %-44s %-32s %s %6.3f s" % (
            c.name, c.M, c.N, c.K, c.layout, c.prec, "x".join(c.cls), c.options(), ";".join(plan), result, time.perf_counter() - t0))


WGRAD_SHAPES = [(1017, [(512, 512), (1536, 512), (512, 2048), (2048, 512)], 0, 0),        # a layer's projections, ragged row count
                (333, [(264, 520), (8, 8), (128, 1000)], 0, 8),                            # partial tiles, padded leading dimensions
                (4097, [(10112, 512)], 3, 0)]                                              # the padded vocabulary, three row ranges


@pytest.mark.parametrize("mode", ["atomics", "workspace"])
@pytest.mark.parametrize("rows,shapes,splitk,ldpad", WGRAD_SHAPES, ids=["ragged_rows", "padded_ld", "three_ranges"])
def test_wgrad_group_exact(L, mode, rows, shapes, splitk, ldpad):
    """ortk_wgrad_group on the S class (rows x 16 < 2^24): dW_i += dY_i^T X_i and db_i += column sums of dY_i, twice onto existing
    integer content, in both reduction forms — equal to the float64 sums bit for bit.  (Three shapes of test_wgrad_group_vs_torch; the
    padding columns of the operands are NaN.)"""
    t0, result = time.perf_counter(), "FAIL"
    try:
        _wgrad_group_exact(L, mode, rows, shapes, splitk, ldpad)
        result = "pass"
    finally:
        _RECORD.append("%-34s rows %5d %s splitk %d ldpad %d S %-9s %s %6.3f s" % (
            "wgrad_group", rows, shapes, splitk, ldpad, mode, result, time.perf_counter() - t0))


def _wgrad_group_exact(L, mode, rows, shapes, splitk, ldpad):
    lib = L.lib()
    a = L.WgradGroupArgs(); a.n = len(shapes); a.rows = rows; a.splitk = splitk
    items = []
    for i, (n, k) in enumerate(shapes):
        key = (rows, i, n, k)
        if key not in _REF:        # operands and the float64 reference once for both reduction forms
            dY, Xm = X.gen_S(rows, n, 31 * i + rows), X.gen_S(rows, k, 31 * i + rows + 1)
            g = torch.Generator().manual_seed(i)
            dW0, db0 = torch.randint(-100, 101, (n, k), generator=g).double(), torch.randint(-100, 101, (n,), generator=g).double()
            _REF[key] = (dY, Xm, dW0, db0, dW0 + 2 * (dY.t() @ Xm), db0 + 2 * dY.sum(0))
            assert 2 * rows * 16 + 100 < X.LIM          # |dY| |X| <= 16 per row, two launches, onto |dW0| <= 100
        dY, Xm, dW0, db0, wantW, wantb = _REF[key]
        _, _, pdy = place(dY, n + ldpad, 0, torch.bfloat16)
        _, _, px = place(Xm, k + ldpad, 0, torch.bfloat16)
        wbuf, wview, pw = place(dW0, k, 0, torch.float32, fill=X.SENTINEL)
        bbuf, bview, pb = place(db0, None, 0, torch.float32, fill=X.SENTINEL)
        it = a.item[i]
        it.dY, it.lddy, it.X, it.ldx, it.dW, it.lddw, it.db, it.Nout, it.Kin = pdy, n + ldpad, px, k + ldpad, pw, k, pb, n, k
        items.append((wbuf, wview, bbuf, bview, wantW, wantb, n, k))
    if mode == "workspace":
        need = lib.ortk_wgrad_group_workspace_bytes(C.byref(a))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda"); _KEEP.append(ws)
        a.ws, a.ws_bytes = ws.data_ptr(), need
    for rep in range(2):          # the second launch adds onto the first (and reuses the workspace)
        L.check(lib.ortk_wgrad_group(C.byref(a), L.stream_ptr()), "ortk_wgrad_group")
    torch.cuda.synchronize()
    for wbuf, wview, bbuf, bview, wantW, wantb, n, k in items:
        assert torch.equal(wview, wantW.float().cuda()), mismatch(wview.cpu().double(), wantW, "dW %d x %d" % (n, k))
        assert torch.equal(bview[0], wantb.float().cuda()), mismatch(bview[0].cpu().double(), wantb, "db %d" % n)
        for buf, cnt in ((wbuf, n * k), (bbuf, n)):
            rest = buf.clone(); rest[SLACK: SLACK + cnt] = X.SENTINEL
            assert bool((rest == X.SENTINEL).all())


def test_the_table_reaches_every_kernel_instance(L):
    """The plans of the whole table (of the cases this session ran, as run; of any other, asked for over stand-in addresses) are exactly
    the instances ortk_gemm.hip can launch: X.INSTANCES, with the exclusions named beside it."""
    seen = set()
    for c in X.CASES:
        plan = _PLANS.get(c.name)
        if plan is None:
            prev = L.set_tuning(**c.tuning)
            try:
                plan = L.gemm_plan(X.fake_args(c, L.GemmArgs()))
            finally:
                L.set_tuning(**prev)
        assert plan == c.plan, c.name
        seen.update(plan)
    assert sorted(seen) == X.INSTANCES
    out = os.environ.get("ORTK_GEMM_EXACT_RECORD")
    if out:        # the per-case record (profiles/gemm_exact_tests.txt)
        with open(out, "w") as f:
            f.write("\n".join(_RECORD) + "\n")
