"""ortk_sparse_build / ortk_spmm on exact operands (tests/spmm_exact.py): integer-valued weights and activations whose partial sums stay
below 2^24, so that the fp32 accumulation of all three formats is exact whatever its order and the result must equal a float64 reference
of the whole epilogue BIT FOR BIT — on a block that is not block 0 of its plan, through every kernel instance, rpw, group split, step
class, staging path and epilogue (ortk_spmm_plan says which form a case runs, and the case asserts it is the one it was built for).
The weight source, X and the epilogue operands sit with padded leading dimensions inside NaN-filled buffers (a read outside the
operand poisons the image or the result), Y inside a sentinel (a write outside (M, N) shows).  No tolerance anywhere in this file."""
import ctypes as C
import os
import time

import pytest
import torch

import gemm_exact as G
import spmm_exact as X
from exact_gpu import NAN, SLACK, _KEEP, mismatch, place
from sparse_decode import ell_to_dense, gu_to_dense

pytestmark = pytest.mark.gpu

_FORMS = {}
_RECORD = []


@pytest.fixture(scope="module")
def L():
    import sparse_image_captioning_amd as P
    P._lib.require_gpu()
    return P._lib


@pytest.fixture(autouse=True)
def release_buffers():
    yield
    del _KEEP[:]


def tdt(d):
    return torch.bfloat16 if d else torch.float32


def place_source(blocks, srcs, dtype):
    """The blocks' source values at their (offset, ld) inside one NaN-filled buffer: the paddings of the leading dimensions, the gaps
    between the blocks and SLACK elements on either side are NaN.  blocks: dicts as SparsePlan takes them.  Returns the tensor the
    builder is handed (offset 0 = its first element)."""
    total = max(b["offset"] + b["N"] * b["ld"] for b in blocks)
    buf = torch.full((SLACK + total + SLACK,), NAN, dtype=dtype, device="cuda")
    for b, src in zip(blocks, srcs):
        at = SLACK + b["offset"]
        buf[at: at + b["N"] * b["ld"]].view(b["N"], b["ld"])[:, :b["K"]] = src.to(dtype).cuda()
    _KEEP.append(buf)
    return buf[SLACK:]


def keep_mask(L, idx, seed):
    """0 / 2 per output element: the draws of ortk_dropout_apply on ones over the index space, taken at each element's index"""
    n = int(idx.max()) + 1
    ones, out = torch.ones(n, device="cuda"), torch.empty(n, device="cuda")
    L.check(L.lib().ortk_dropout_apply(L.ptr(ones), L.ptr(out), 0, n, X.DROP_P, seed, L.stream_ptr()), "ortk_dropout_apply")
    torch.cuda.synchronize()
    k = out[idx.cuda()].cpu().double()
    assert set(k.unique().tolist()) <= {0.0, 2.0}
    return k


def sentinel_intact(buf, off, M, ld, N):
    rest = buf.clone()
    rest[SLACK + off: SLACK + off + M * ld].view(M, ld)[:, :N] = X.SENTINEL
    return bool((rest == X.SENTINEL).all())


def run_case(L, c):
    from sparse_image_captioning_amd.sparse import SparsePlan
    o = X.operands(c)
    blocks = X.block_dicts(c, o)
    plan = SparsePlan(blocks, c.fmt, "cuda")
    plan.build(place_source(blocks, o["Wsrc"], tdt(c.wdt)))
    if c.fmt != X.GU16:
        plan.check_overflow()
    ldx, ldy, ldr, ldg = X.lds(c)
    ptr = {}
    _, _, ptr["X"] = place(o["A"], ldx, c.off[0], tdt(c.xdt))
    eo = c.off[2]
    for k, ld, d in (("bias", None, 0), ("rowscale", None, 0), ("resid", ldr, 0), ("gate", ldg, int(c.gate == "bf16"))):
        if k in o:
            _, _, ptr[k] = place(o[k], ld, eo, tdt(d))
    if "rows" in o:
        _, _, ptr["rows"] = place(o["rows"], None, 0, torch.int32, fill=0)
    seed = 1000 + c.seed % 1000
    keep = keep_mask(L, X.drop_index(c, o), seed) if c.drop else None
    want, _ = G.expected(c, o, keep)
    want32 = want.float()
    assert torch.equal(want32.double(), want)                      # (the reference itself is an exact fp32 value)
    want_dev = (want32.bfloat16() if c.ydt else want32).cuda()     # a bf16 Y: the exact fp32 result, rounded by torch

    def launch():
        ybuf, yview, ptr["Y"] = place(torch.full((c.M, c.N), X.SENTINEL, dtype=torch.float64), ldy, c.off[1], tdt(c.ydt), fill=X.SENTINEL)
        a = X.fill_args(c, L.SpmmArgs(), ptr)
        form = L.spmm_plan(plan, c.call, a)
        assert form == c.form, (c.name, form)
        plan.spmm(c.call, a)
        torch.cuda.synchronize()
        return form, ybuf, yview

    prev = L.set_tuning(**c.tuning)
    try:
        form, ybuf, yview = launch()
        again = launch()
    finally:
        L.set_tuning(**prev)
    _FORMS[c.name] = form
    if c.fmt == X.GU16:       # the bound the builder left for THIS block, and the unrolled body it selects
        got = int(plan.perm[c.call])
        assert got == X.gu_bound(o["B"]) and X.step_class(got) == c.steps, (c.name, got)
    assert torch.equal(yview, want_dev), mismatch(yview.cpu(), want_dev.cpu(), c.name)
    assert sentinel_intact(ybuf, c.off[1], c.M, ldy, c.N), c.name + ": written outside (M, N)"
    bits = torch.int16 if c.ydt else torch.int32
    assert torch.equal(again[1].view(bits), ybuf.view(bits)), c.name + ": rerun differs"
    return form


@pytest.mark.parametrize("c", X.CASES, ids=lambda c: c.name)
def test_spmm_exact(L, c):
    t0, form, result = time.perf_counter(), c.form, "FAIL"
    try:
        form = run_case(L, c)
        result = "pass"
    finally:          # (a failing case leaves its line too, with the form it was built for)
        _RECORD.append("%-28s %-5s %-52s %-10s %-66s %-52s %s %6.3f s" % (
            c.name, X.FMT[c.fmt], c.shapes(), "x".join(c.cls), c.options(), form + (" steps=%d" % c.steps if c.steps else ""), result,
            time.perf_counter() - t0))


def product(L, plan, bi, A, xdt=1, resid_in_place=None, koff=0):
    """Y = A[:, koff: koff + K] W~^T of block bi (K its inputs), plain epilogue: X with ldx = A's width + 8 (NaN behind every row) inside a
    NaN buffer, fp32 Y inside the sentinel; resid_in_place = (buffer, view, address) of an earlier product: accumulate onto it.
    Returns ((buffer, view, address), ldy, the plan string)."""
    N = plan.blocks[bi]["N"]
    M = A.shape[0]
    ldx, ldy = A.shape[1] + 8, N + 4
    _, _, px = place(A, ldx, 0, tdt(xdt))
    a = L.SpmmArgs()
    if resid_in_place is None:
        ybuf, yview, py = place(torch.full((M, N), X.SENTINEL, dtype=torch.float64), ldy, 0, torch.float32, fill=X.SENTINEL)
    else:
        ybuf, yview, py = resid_in_place
        a.resid, a.ldr = py, ldy
    a.X, a.Y, a.ldx, a.ldy, a.M, a.x_dtype, a.y_dtype = px + koff * (2 if xdt else 4), py, ldx, ldy, M, xdt, 0
    form = L.spmm_plan(plan, bi, a)
    plan.spmm(bi, a)
    torch.cuda.synchronize()
    return (ybuf, yview, py), ldy, form


def decode(plan, bi):
    return torch.from_numpy((gu_to_dense if plan.format == X.GU16 else ell_to_dense)(plan, bi)).double()


def check_block(L, plan, bi, W, A, what):
    """The image of block bi decodes to exactly W and its product with A is exact."""
    got = decode(plan, bi)
    assert torch.equal(got, W), mismatch(got, W, what + ": image")
    (ybuf, yview, _), ldy, _ = product(L, plan, bi, A, xdt=0 if plan.format == X.ELL32 else 1)
    want = (A @ W.t()).float().cuda()
    assert torch.equal(yview, want), mismatch(yview.cpu(), want.cpu(), what + ": product")
    assert sentinel_intact(ybuf, 0, A.shape[0], ldy, W.shape[0]), what


@pytest.mark.parametrize("fmt", [X.ELL32, X.ELL16, X.GU16], ids=lambda f: X.FMT[f])
def test_rebuild_with_a_different_pattern(L, fmt):
    """One plan, three builds: a dense-ish matrix, a much sparser one with a different support, the first again (a training step rebuilds
    the images from a new mask sample every step).  After each build both blocks decode to exactly the matrix just built — no stale
    entry of a denser pattern — the products are exact, and the GU16 step bound of the rebuilt block is the new matrix's own."""
    from sparse_image_captioning_amd.sparse import SparsePlan
    N, K = 132, 520 if fmt == X.GU16 else 264
    blk = [X.B(48, 72, "b80", pad=3, gap=5), X.B(N, K, "b50", pad=8, gap=8)]
    c = X.Case("rebuild_%d" % fmt, fmt, blk, 17, "", steps=0 if fmt == X.GU16 else None)
    o = X.operands(c)
    Wa = o["W"][1]
    Wb = X.gen_block(X.B(N, K, "b99"), "S", 4242)[0]
    assert ((Wa != 0) & (Wb != 0)).sum() < (Wb != 0).sum() < 0.05 * (Wa != 0).sum()      # B: much sparser, mostly outside A's support
    blocks = [dict(d, capacity=X.capacity(c, b, Wa if i else o["W"][0])) for i, (d, b) in enumerate(zip(X.block_dicts(c, o), blk))]
    plan = SparsePlan(blocks, fmt, "cuda")
    A = o["A"]
    A0 = X.gen_S(17, 72, 5)
    for step, W in enumerate((Wa, Wb, Wa)):
        plan.build(place_source(blocks, [o["W"][0].float(), W.float()], torch.float32 if step != 1 else torch.bfloat16))
        if fmt != X.GU16:
            plan.check_overflow()
        check_block(L, plan, 1, W, A, "build %d" % step)
        check_block(L, plan, 0, o["W"][0], A0, "build %d, block 0" % step)
        if fmt == X.GU16:
            assert int(plan.perm[1]) == X.gu_bound(W) and int(plan.perm[0]) == X.gu_bound(o["W"][0])
    if fmt == X.GU16:
        assert X.step_class(X.gu_bound(Wa)) == 16 and X.step_class(X.gu_bound(Wb)) == 8


@pytest.mark.parametrize("fmt", [X.ELL32, X.ELL16], ids=lambda f: X.FMT[f])
def test_ell_overflow_leaves_the_neighbour_alone(L, fmt):
    """Block 0 denser than its capacity, block 1 sized normally: the overflow is reported, block 0 holds a subset of its weights (each
    stored once, with its value) and multiplies by exactly that subset, and block 1 — image words, chunk tables, product — is what the
    same plan with room for block 0 builds."""
    from sparse_image_captioning_amd.sparse import SparsePlan
    blk = [X.B(132, 72, "b50", pad=3, gap=5), X.B(70, 40, "b80", pad=8, gap=8)]
    c = X.Case("overflow_%d" % fmt, fmt, blk, 17, "")
    o = X.operands(c)
    W0, W1 = o["W"]
    roomy = X.block_dicts(c, o)
    tight = [dict(roomy[0], capacity=64 * 8 * 3), roomy[1]]
    assert tight[0]["capacity"] < int((W0 != 0).sum())
    plans = []
    for blocks in (tight, roomy):
        plan = SparsePlan(blocks, fmt, "cuda")
        plan.build(place_source(blocks, o["Wsrc"], torch.float32))
        plans.append(plan)
    small, big = plans
    with pytest.raises(L.OrtkError):
        small.check_overflow()
    big.check_overflow()
    A1, A0 = o["A"], X.gen_S(17, 72, 5)
    check_block(L, small, 1, W1, A1, "the neighbour")
    check_block(L, big, 0, W0, A0, "block 0 with room")
    # block 1's share of the tables and of the stream, word for word (its chunk offsets relative to its own region)
    wpe = 1 if fmt == X.ELL16 else 2            # 32-bit words per entry
    for p in plans:
        h = p._host[1]
        c0, nch = h.chunk0, (h.N + 63) // 64
        p.words = p.stream[h.stream_offset * wpe: (h.stream_offset + h.capacity) * wpe].cpu()
        p.ptrs = (p.chunk_ptr[c0: c0 + nch] - h.stream_offset).cpu()
        p.lens = p.chunk_len[c0: c0 + nch].cpu()
        p.lanes = p.perm[c0 * 64: (c0 + nch) * 64].cpu()
    assert torch.equal(small.words, big.words) and torch.equal(small.ptrs, big.ptrs)
    assert torch.equal(small.lens, big.lens) and torch.equal(small.lanes, big.lanes)
    # block 0: a subset (the decoder asserts that no position is stored twice), and the product of exactly that subset
    sub = decode(small, 0)
    held = sub != 0
    assert torch.equal(sub[held], W0[held]) and 0 < int(held.sum()) < int((W0 != 0).sum())
    (ybuf, yview, _), ldy, _ = product(L, small, 0, A0, xdt=0 if fmt == X.ELL32 else 1)
    want = (A0 @ sub.t()).float().cuda()
    assert torch.equal(yview, want), mismatch(yview.cpu(), want.cpu(), "the cut block's product")
    assert sentinel_intact(ybuf, 0, 17, ldy, 132)


@pytest.mark.parametrize("fmt", [X.ELL16, X.GU16], ids=lambda f: X.FMT[f])
def test_the_executor_piece_layout(L, fmt):
    """The data gradient of a wide projection as the executor cuts it: ONE dense (N, Kw) matrix, a two-block plan of its 2 048-wide
    pieces (ld = Kw, offsets 0 and 2 048), two products over X + k0 with ldx = Kw, the second accumulating in place (resid == Y):
    Y is the whole product, exactly."""
    from sparse_image_captioning_amd.sparse import SparsePlan
    N, Kw, M = 512, 2048 + 520, 33
    W = X.gen_block(X.B(N, Kw, "b95"), "S", 77)[0]
    A = X.gen_S(M, Kw, 78)
    assert (A.abs() @ W.abs().t()).max().item() < X.LIM
    c = X.Case("pieces_%d" % fmt, fmt, [X.B(N, 2048, "b95"), X.B(N, 520, "b95")], M, "", steps=0 if fmt == X.GU16 else None)
    pieces = [W[:, :2048], W[:, 2048:]]
    blocks = [dict(offset=k0, N=N, K=p.shape[1], ld=Kw, capacity=X.capacity(c, b, p)) for k0, p, b in zip((0, 2048), pieces, c.blocks)]
    plan = SparsePlan(blocks, fmt, "cuda")
    src = torch.full((SLACK + N * Kw + SLACK,), NAN, dtype=torch.bfloat16, device="cuda")
    src[SLACK: SLACK + N * Kw] = W.bfloat16().reshape(-1).cuda()
    _KEEP.append(src)
    plan.build(src[SLACK:])
    if fmt != X.GU16:
        plan.check_overflow()
    want_form = "ell<bf16,2048,512,1>:rpw=1:stage=fast:epi=lean" if fmt == X.ELL16 else "gu<1,1>:gsplit=8:stage=fast:epi=lean"
    # (product() places A with ldx = Kw + 8: a padded row pitch, as the executor's lddy is for the generator)
    y, ldy, form0 = product(L, plan, 0, A)
    first = (A[:, :2048] @ pieces[0].t()).float().cuda()
    assert torch.equal(y[1], first), mismatch(y[1].cpu(), first.cpu(), "first piece")
    _, _, form1 = product(L, plan, 1, A, resid_in_place=y, koff=2048)
    assert (form0, form1) == (want_form, want_form)
    want = (A @ W.t()).float().cuda()
    assert torch.equal(y[1], want), mismatch(y[1].cpu(), want.cpu(), "both pieces")
    assert sentinel_intact(y[0], 0, M, ldy, N)


def test_refusals_launch_nothing(L):
    """What ortk_spmm and ortk_sparse_build refuse is ORTK_EINVAL before any launch: Y and the images keep their bytes."""
    from sparse_image_captioning_amd.sparse import SparsePlan
    lib = L.lib()
    A = X.gen_S(17, 520, 1)
    _, _, px = place(A, 528, 0, torch.bfloat16)
    ybuf, _, py = place(torch.full((17, 600), X.SENTINEL, dtype=torch.float64), 600, 0, torch.float32, fill=X.SENTINEL)

    def args(**kw):
        a = L.SpmmArgs()
        a.X, a.Y, a.ldx, a.ldy, a.M, a.x_dtype, a.y_dtype = px, py, 528, 600, 17, 1, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(plan, block, a):
        buf = C.create_string_buffer(128)
        return (lib.ortk_spmm(plan.ref(), block, C.byref(a), L.stream_ptr()), lib.ortk_spmm_plan(plan.ref(), block, C.byref(a), buf, 128)) == (-1, -1)

    src = torch.zeros(1200 * 2100, device="cuda")
    # ---- a good two-block plan: block out of range, dtypes outside {0, 1}
    for fmt in (X.ELL32, X.ELL16, X.GU16):
        plan = SparsePlan([dict(offset=0, N=70, K=40, ld=40, capacity=64 * 8 * 2), dict(offset=2800, N=132, K=520, ld=520, capacity=64 * 8 * 3)], fmt, "cuda")
        plan.build(src)
        assert refused(plan, 2, args()) and refused(plan, -1, args())
        assert refused(plan, 1, args(x_dtype=2)) and refused(plan, 1, args(y_dtype=-1)) and refused(plan, 1, args(gate_dtype=2))
        assert refused(plan, 1, args(M=-1)) and refused(plan, 1, args(X=0)) and refused(plan, 1, args(Y=0))
        plan.stream.fill_(7)
        assert lib.ortk_sparse_build(plan.ref(), L.ptr(src), 2, L.stream_ptr()) == -1
        torch.cuda.synchronize()
        assert bool((plan.stream == 7).all())
    # ---- a GU16 block with K > 512 and N > 512 (the table is edited behind SparsePlan, whose buffers stay large enough for it)
    plan = SparsePlan([dict(offset=0, N=16, K=8, ld=8), dict(offset=128, N=512, K=1030, ld=1030)], X.GU16, "cuda")
    h = plan._host[1]
    h.N, h.K, h.ld = 528, 520, 520
    plan.struct.total_rows = 1 + 33 * 2
    plan.stream.fill_(7.0)
    assert lib.ortk_sparse_build(plan.ref(), L.ptr(src), 0, L.stream_ptr()) == -1
    assert refused(plan, 1, args())
    torch.cuda.synchronize()
    assert bool((plan.stream == 7.0).all())
    # ---- an ELL block with K > 2 048
    for fmt in (X.ELL32, X.ELL16):
        plan = SparsePlan([dict(offset=0, N=70, K=40, ld=40, capacity=1024), dict(offset=2800, N=64, K=2048, ld=2100, capacity=1024)], fmt, "cuda")
        plan._host[1].K = 2049
        plan.stream.fill_(7)
        assert lib.ortk_sparse_build(plan.ref(), L.ptr(src), 0, L.stream_ptr()) == -1
        assert refused(plan, 1, args())
        torch.cuda.synchronize()
        assert bool((plan.stream == 7).all())
    torch.cuda.synchronize()
    assert bool((ybuf == X.SENTINEL).all())


def test_the_table_reaches_every_kernel_form(L):
    """The plan strings of the whole table (of the cases this session ran, as run; of any other, asked for over stand-in addresses)
    cover exactly X.FORMS: the 18 kernel instances, every rpw, every GU16 step class, both staging paths and both epilogues per format."""
    seen = set()
    for c in X.CASES:
        form = _FORMS.get(c.name)
        if form is None:
            form = X.plan_string(L, c)
        assert form == c.form, c.name
        seen |= X.features(c, form)
    assert sorted(seen) == X.FORMS and not seen & set(X.EXCLUDED)
    out = os.environ.get("ORTK_SPMM_EXACT_RECORD")
    if out:        # the per-case record (profiles/spmm_exact_tests.txt)
        with open(out, "w") as f:
            f.write("\n".join(_RECORD) + "\n")
            f.write("%d cases, %.1f s in them\n" % (len(_RECORD), sum(float(r.split()[-2]) for r in _RECORD)))
