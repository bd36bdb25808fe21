"""The rows-stationary chain kernels (csrc/ortk_chain.hip: row_chain_kernel, row_chain_wide_kernel, row_bchain_kernel) on a real MI355X
against the float64 reference, the fp32 error model and the exact routing operands of tests/chain_ref.py (read its docstring first).
tests/test_chain_ref_host.py shows on the CPU that the bars are sound and sharp, and that the geometry table below is what the
launcher does.

Every buffer a kernel reads or writes is a slice of a NaN-filled allocation with fences (test_gpu_layernorm.Fenced): the fences are
asserted intact after every call -- rows past M, the pad columns of out1 / out2 where ld = 512 n + 8, the buffers next to each output --
and every output is asserted finite (a read past an input, a stale or a never-written entry reaches an output as NaN).  Every case
asserts its plan (ortk_row_chain_plan: kernel form, rows per block, workgroups, prefetchers) BEFORE it runs, and runs twice into
NaN-refilled outputs: the two results are the same bytes (the backward's da / db, which arrive by float atomics, within the rerun
bound of the LayerNorm tests).

Each stage is compared with the float64 evaluation of ITS OWN stored input (chain_ref.forward_stages / backward_stages): fp32 outputs
within 4 bounds, bf16 outputs inside their rounding interval.  The reference is numpy float64 on the CPU up to 4 200 rows and torch
float64 on the device above (test_device_reference_agrees_with_cpu holds the second to the first).  The LayerNorm inputs are
ln_ref.class_rows.  Each test prints its largest error / bound per output (profiles/row_chain_operator_tests.txt)."""
import ctypes as C

import numpy as np
import pytest
import torch

import chain_ref as CR
import ln_ref as R
from test_gpu_layernorm import Fenced

pytestmark = pytest.mark.gpu

D = 512
F32 = np.float32
CPU_ROWS = 4200                  # the reference is numpy float64 on the CPU up to here
SEEDS = dict(r=1111, h=2222, o=3333, a=4321, b=8765)
CLASS_SCALE = np.array([2.0, 2.0, 1e-3, 1e-6, 1e-3])
FULL = dict(R=1, n1=3, F=1, L2=1, n2=3)


@pytest.fixture(scope="module")
def L():
    import sparse_image_captioning_amd as P
    P._lib.require_gpu()
    return P._lib


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _nan(n):
    return torch.full((int(n),), float("nan"))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y))


def _bf(x):
    return CR.bf16_rn(np.asarray(x, dtype=F32))


def _keep(L, seed, keys, Mk, ncols, p):
    """(rows, ncols) fp32 on the device: 0 or the kernels' 1 / (1 - p), the draws of rows `keys` of a (Mk, ncols) tensor, from
    ortk_dropout_apply on ones."""
    if p == 0:
        return torch.ones(len(keys), ncols, device="cuda")
    ones, out = torch.ones(Mk * ncols, device="cuda"), torch.empty(Mk * ncols, device="cuda")
    L.check(L.lib().ortk_dropout_apply(L.ptr(ones), L.ptr(out), 0, Mk * ncols, p, seed, L.stream_ptr()), "ortk_dropout_apply")
    return out.view(Mk, ncols)[torch.as_tensor(keys, device="cuda", dtype=torch.long)]


_OPERANDS = {}


def _operands(form, NC, routing):
    """The weights and vectors of a chain (numpy; cached: the same for every row count) and, for routing, the selection tables."""
    key = (tuple(sorted(form.items())), NC, routing)
    if key in _OPERANDS:
        return _OPERANDS[key]
    g = np.random.default_rng(1000 + NC)
    ff = NC * D
    vec = lambda n, sc=0.1: (sc * g.standard_normal(n)).astype(F32)
    mk = lambda n, k: _bf(g.standard_normal((n, k)) * (0.5 / np.sqrt(k)))
    w, rt = {}, {}
    w.update(g1=(1 + vec(D)).astype(F32), b1=vec(D))
    zero_bias = bool(routing)
    if form["R"]:
        if routing:
            w["Wr"], *rt["Wr"] = CR.routing_unit(11)
        else:
            w["Wr"] = mk(D, D)
        w["bias_r"] = np.zeros(D, F32) if zero_bias else vec(D)
    if form["n1"]:
        if routing:
            w["S1"], *rt["S1"] = CR.routing_stack(form["n1"], 12)
        else:
            w["S1"] = mk(form["n1"] * D, D)
        w["bias_s1"] = np.zeros(form["n1"] * D, F32) if zero_bias else vec(form["n1"] * D)
    if form["F"]:
        if routing:
            w["W1"], *rt["W1"] = CR.routing_stack(NC, 13)
            w["W2"], *rt["W2"] = CR.routing_w2(NC, 14)
        else:
            w["W1"], w["W2"] = mk(ff, D), mk(D, ff)
        w["bias_h"], w["bias_o"] = vec(ff), vec(D)
        if routing == "mask":      # every hidden unit active, no entry of the two residual updates zero or absorbed (see the mask test)
            w["bias_h"] = (32 + vec(ff)).astype(F32)
            w["bias_o"] = (np.sign(g.standard_normal(D)) * (0.05 + np.abs(vec(D)))).astype(F32)
    if form["L2"]:
        w.update(g2=(1 + vec(D)).astype(F32), b2=vec(D))
    if form["n2"]:
        if routing:
            w["S2"], *rt["S2"] = CR.routing_stack(form["n2"], 15)
        else:
            w["S2"] = mk(form["n2"] * D, D)
        w["bias_s2"] = np.zeros(form["n2"] * D, F32) if zero_bias else vec(form["n2"] * D)
    rt = {k: tuple(v) for k, v in rt.items()}
    for k in ("bias_r", "bias_h", "bias_o"):
        if k in w:
            rt[k] = w[k]
    _OPERANDS[key] = (w, rt)
    return w, rt


class FwdCase:
    """One forward chain: inputs, fenced buffers, arguments; run() launches it and returns the stored outputs (device tensors)."""

    def __init__(self, L, M, form=FULL, NC=4, p=0.1, routing=False, keyed=None, progress=False, ld_pad=0, eps=1e-6, chain_wide=1):
        self.L, self.M, self.form, self.NC, self.p, self.eps = L, M, form, (NC if form["F"] else 0), p, eps
        self.routing, self.progress, self.chain_wide = routing, progress, chain_wide
        NC, ff = self.NC, self.NC * D
        self.w, self.rt = _operands(form, NC, routing)
        w = self.w
        g = np.random.default_rng(M)
        rows, kind = R.class_rows(M, D, M)
        a = g.standard_normal((M, D))
        if routing == "mask":
            a = np.sign(a) * (0.5 + np.abs(a))
        self.kind, self.a_in = kind, _bf(a * CLASS_SCALE[kind][:, None])
        # ---- dropout keys: rows of a taller tensor
        self.Mk, self.keys = M, np.arange(M)
        if keyed:
            self.Mk = M + 500
            if keyed == "subset":
                self.keys = np.sort(g.permutation(self.Mk)[:M])
            else:                  # "tail": the rows of the partial last block alone are keyed elsewhere
                last = CR.plan(M, chain_wide, progress)["last"]
                self.keys = np.arange(M); self.keys[M - last:] += 500 - 1
            self.key_dev = torch.tensor(self.keys, dtype=torch.int32).cuda()
        # ---- the residual rows: chosen so that the FIRST LayerNorm's input is the class rows -- with R, x_in = rows - the update R adds
        #      (float64, rounded once; a_in is scaled by the row's class, so the update's own rounding, u |bias_r|, stays below the
        #      spread of the narrowest class).  The second LayerNorm's input, x_out, is of class 0 whatever comes in, except in the
        #      form without F, where it is these rows again.
        x_in = rows
        if form["R"]:
            k = CR.keep(SEEDS["r"], self.keys, D, p) * float(CR.keep_scale(p)) if p > 0 else 1.0
            x_in = (rows.astype(np.float64) - k * (self.a_in.astype(np.float64) @ w["Wr"].astype(np.float64).T + w["bias_r"])).astype(F32)
        self.x_in = x_in
        # ---- the bf16 arena and the unit table, in stream order
        names = [n for n in ("Wr", "S1", "W1", "W2", "S2") if n in w]
        off, cur = {}, 0
        for n in names:
            off[n] = cur
            cur += w[n].size
        self.f_arena = Fenced([_t(np.concatenate([w[n].reshape(-1) for n in names]))], torch.bfloat16)
        units = [(off["Wr"], D)] if form["R"] else []
        units += [(off["S1"] + i * D * D, D) for i in range(form["n1"])]
        for c in range(NC):
            units += [(off["W1"] + c * D * D, D), (off["W2"] + c * D, ff)]
        units += [(off["S2"] + i * D * D, D) for i in range(form["n2"])]
        self.units = torch.tensor(units, dtype=torch.int64).cuda()
        nb = L.lib().ortk_chain_packed_bytes(len(units))
        self.f_packed = Fenced([_nan(nb // 2)], torch.bfloat16)
        # ---- inputs
        self.f_x = Fenced([_t(x_in)])
        self.f_a = Fenced([_t(self.a_in)], torch.bfloat16)
        vn = [n for n in ("bias_r", "g1", "b1", "bias_s1", "bias_h", "bias_o", "g2", "b2", "bias_s2") if n in w]
        self.f_v = Fenced([_t(w[n]) for n in vn])
        self.vec = dict(zip(vn, self.f_v.views))
        # ---- outputs
        self.ld1, self.ld2 = form["n1"] * D + ld_pad, form["n2"] * D + ld_pad
        self.f_o32 = Fenced([_nan(M * D), _nan(M * D), _nan(M * 2), _nan(M * 2)])
        self.f_o16 = Fenced([_nan(M * D), _nan(M * D), _nan(M * max(self.ld1, 8)), _nan(M * max(self.ld2, 8)), _nan(M * max(ff, 8))], torch.bfloat16)
        # ---- progress: 16 ints with 8 sentinels on both sides
        self.prog = torch.full((32,), -7, dtype=torch.int32, device="cuda")
        self.null = ()

    def args(self):
        L, w, form, M = self.L, self.w, self.form, self.M
        a = L.ChainArgs()
        a.w16, a.units_dev, a.n_units = L.ptr(self.f_arena.views[0]), self.units.data_ptr(), self.units.shape[0]
        a.packed, a.packed_bytes = L.ptr(self.f_packed.views[0]), self.f_packed.views[0].numel() * 2
        a.M, a.x_in = M, L.ptr(self.f_x.views[0])
        x_mid, x_out, st1, st2 = self.f_o32.views
        y1, y2, out1, out2, h = self.f_o16.views
        P = lambda name, t: None if name in self.null else L.ptr(t)
        if form["R"]:
            a.a_in, a.bias_r, a.x_mid, a.seed_r = L.ptr(self.f_a.views[0]), L.ptr(self.vec["bias_r"]), L.ptr(x_mid), SEEDS["r"]
        a.g1, a.b1, a.y1, a.st1 = L.ptr(self.vec["g1"]), L.ptr(self.vec["b1"]), P("y1", y1), P("st1", st1)
        a.n1 = form["n1"]
        if form["n1"]:
            a.bias_s1, a.out1, a.ld1 = L.ptr(self.vec["bias_s1"]), L.ptr(out1), self.ld1
        if form["F"]:
            a.NC, a.bias_h, a.bias_o, a.h, a.x_out = self.NC, L.ptr(self.vec["bias_h"]), L.ptr(self.vec["bias_o"]), P("h", h), L.ptr(x_out)
            a.seed_h, a.seed_o = SEEDS["h"], SEEDS["o"]
        if form["L2"]:
            a.g2, a.b2, a.y2, a.st2 = L.ptr(self.vec["g2"]), L.ptr(self.vec["b2"]), P("y2", y2), P("st2", st2)
        a.n2 = form["n2"]
        if form["n2"]:
            a.bias_s2, a.out2, a.ld2 = L.ptr(self.vec["bias_s2"]), L.ptr(out2), self.ld2
        a.drop_p, a.eps = self.p, self.eps
        if self.Mk != M:
            a.drop_rows = self.key_dev.data_ptr()
        if self.progress:
            a.progress = self.prog[8:].data_ptr()
        return a

    def present(self):
        f = self.form
        names = (["x_mid"] if f["R"] else []) + ["y1", "st1"] + (["out1"] if f["n1"] else []) + (["h", "x_out"] if f["F"] else [])
        names += (["y2", "st2"] if f["L2"] else []) + (["out2"] if f["n2"] else [])
        return [n for n in names if n not in self.null]

    def run(self, null=()):
        """Plan asserted, outputs refilled with NaN, one launch, fences and finiteness asserted; returns {name: device tensor}."""
        L, M, f = self.L, self.M, self.form
        self.null = tuple(null)
        a = self.args()
        want = CR.plan(M, self.chain_wide, self.progress)
        got = L.row_chain_plan(a)
        assert got == {k: want[k] for k in got}, (got, want)
        self.f_o32.buf.fill_(float("nan")); self.f_o16.buf.fill_(float("nan")); self.f_packed.buf.fill_(float("nan"))
        L.check(L.lib().ortk_row_chain(C.byref(a), L.stream_ptr()), "ortk_row_chain")
        torch.cuda.synchronize()
        for fb in (self.f_arena, self.f_packed, self.f_x, self.f_a, self.f_v, self.f_o32, self.f_o16):
            assert fb.intact(), "a fence is broken: the chain wrote outside its outputs"
        x_mid, x_out, st1, st2 = self.f_o32.views
        y1, y2, out1, out2, h = self.f_o16.views
        full = dict(x_mid=x_mid.view(M, D), x_out=x_out.view(M, D), st1=st1.view(M, 2), st2=st2.view(M, 2), y1=y1.view(M, D), y2=y2.view(M, D),
                    out1=out1.view(M, -1), out2=out2.view(M, -1), h=h.view(M, -1))
        s = {}
        for n, v in full.items():
            if n in self.present():
                if n in ("out1", "out2"):
                    nn = f["n1" if n == "out1" else "n2"] * D
                    assert torch.isnan(v[:, nn:]).all(), f"{n}: a pad column was written"
                    v = v[:, :nn]
                assert torch.isfinite(v).all(), f"{n}: not every entry written, or something read past an input / a stale row"
                s[n] = v.clone()
            else:
                assert torch.isnan(v).all(), f"{n} is not an output of this form, and it was written"
        if self.progress:
            pr, n_units = self.prog.cpu(), a.n_units
            assert (pr[:8] == -7).all() and (pr[24:] == -7).all(), "the progress array's neighbours were written"
            assert (pr[17:24] == 0).all() and int(pr[16]) in (0, 1)
            for x in range(8):           # XCD x: the last store of one of its pace-makers (block x of a round), 0 where it has none
                ok = {n_units * (r + 1) for r in range(want["rounds"]) if x + 248 * r < want["workgroups"]} or {0}
                assert int(pr[8 + x]) in ok, (x, int(pr[8 + x]), ok)
        self.plan_ = want
        return s

    def stages(self, s, device=None):
        t = dict(x_in=self.f_x.views[0].view(self.M, D), a_in=self.f_a.views[0].view(self.M, D))
        t.update(s)
        w = dict(self.w)
        if self.p > 0:
            if self.form["R"]: w["keep_r"] = _keep(self.L, SEEDS["r"], self.keys, self.Mk, D, self.p)
            if self.form["F"]:
                w["keep_h"] = _keep(self.L, SEEDS["h"], self.keys, self.Mk, self.NC * D, self.p)
                w["keep_o"] = _keep(self.L, SEEDS["o"], self.keys, self.Mk, D, self.p)
        self.w_keep = w
        return CR.forward_stages(t, w, self.p, self.eps, device=device)

    def check(self, tag, s=None, twice=True):
        s = self.run() if s is None else s
        dev = "cuda" if self.M > CPU_ROWS else None
        res = CR.check(s, self.stages(s, dev), f"{tag} M={self.M} p={self.p} {self.plan_}")
        if twice:
            s2 = self.run()
            for n in s:
                assert _same(s[n], s2[n]), f"{n}: a rerun changed bits"
        return s, res


def _tuned(L, chain_wide):
    return L.set_tuning(chain_wide=chain_wide)


# ------------------------------------------------------------------------------------------------ forward: geometry classes
@pytest.mark.parametrize("p", [0.1, 0.0])
@pytest.mark.parametrize("case", sorted(CR.GEOMETRY_CASES), ids=lambda c: f"M{c[0]}-wide{c[1]}-pf{c[2]}")
def test_forward_geometry(L, case, p):
    """The full chain R L1 S1(3) F L2 S2(3), NC = 4, at every block height class of both kernel forms, the two-round grids and the
    prefetcher grid (chain_ref.GEOMETRY_CASES); ld = 512 n + 8 in every second case."""
    M, cw, pf = case
    old = _tuned(L, cw)
    try:
        c = FwdCase(L, M, p=p, progress=bool(pf), ld_pad=8 if sorted(CR.GEOMETRY_CASES).index(case) % 2 else 0, chain_wide=cw)
        form, rb, wg, last = CR.GEOMETRY_CASES[case]
        c.check("geometry")
        assert (c.plan_["form"], c.plan_["rows_per_block"], c.plan_["workgroups"], c.plan_["last"]) == (form, rb, wg, last)
    finally:
        L.set_tuning(**old)


# ------------------------------------------------------------------------------------------------ forward: argument forms
FORMS = {
    "L1 S1(3)": dict(R=0, n1=3, F=0, L2=0, n2=0),
    "R L1 S1(1)": dict(R=1, n1=1, F=0, L2=0, n2=0),
    "R L1 F L2": dict(R=1, n1=0, F=1, L2=1, n2=0),
    "L1 F L2 S2(3)": dict(R=0, n1=0, F=1, L2=1, n2=3),
    "R L1 S1(2)": dict(R=1, n1=2, F=0, L2=0, n2=0),
    "R L1 S1(3) F L2 S2(1)": dict(R=1, n1=3, F=1, L2=1, n2=1),
    "R L1 S1(3) F L2 S2(2)": dict(R=1, n1=3, F=1, L2=1, n2=2),
    "L1 S1(1) L2 S2(1)": dict(R=0, n1=1, F=0, L2=1, n2=1),            # no F: the second LayerNorm sees the class rows too
}
FORM_ROWS = (257, 4100, 12289)


@pytest.mark.parametrize("M", FORM_ROWS)
@pytest.mark.parametrize("name", sorted(FORMS))
def test_forward_forms(L, name, M):
    c = FwdCase(L, M, form=FORMS[name], p=0.1, ld_pad=8 if (sorted(FORMS).index(name) + M) % 2 else 0)
    c.check(name)
    assert c.plan_["form"] == int(M == 12289)


@pytest.mark.parametrize("M", FORM_ROWS)
@pytest.mark.parametrize("NC", [1, 8])
def test_forward_chunk_counts(L, NC, M):
    FwdCase(L, M, NC=NC, p=0.1).check(f"NC={NC}")


@pytest.mark.parametrize("M", FORM_ROWS)
def test_forward_null_outputs(L, M):
    """h, y1, st1, st2 NULL one at a time and all together (and y2 with them: the inference form): nothing is written for them, and
    every remaining output is the same bytes as in the full form."""
    c = FwdCase(L, M, p=0.1)
    s, _ = c.check("full form of the NULL cases", twice=False)
    for null in (("h",), ("y1",), ("st1",), ("st2",), ("h", "y1", "st1", "st2"), ("h", "y1", "st1", "st2", "y2")):
        s2 = c.run(null=null)
        assert set(s2) == set(s) - set(null)
        for n in s2:
            assert _same(s[n], s2[n]), f"{n} changed with {null} NULL"


@pytest.mark.parametrize("M,keyed", [(257, "subset"), (4100, "subset"), (4100, "tail"), (12289, "subset"), (16385, "tail")])
def test_forward_drop_rows(L, M, keyed):
    """ortk_chain_args.drop_rows: rows keyed into a taller tensor, on both kernel forms; "tail" keys the rows of the partial last
    block alone elsewhere (3 rows at 4 100, 5 at 16 385), so that a key taken from a neighbouring row shows."""
    c = FwdCase(L, M, p=0.1, keyed=keyed)
    c.check(f"drop_rows {keyed}")
    if keyed == "tail":
        assert c.plan_["last"] in (3, 5) and (c.keys[-c.plan_["last"]:] >= M).all()


def test_forward_eps(L):
    FwdCase(L, 257, p=0.1, eps=1e-3).check("eps=1e-3")
    FwdCase(L, 12289, p=0.0, eps=1e-5).check("eps=1e-5")


def test_device_reference_agrees_with_cpu(L):
    """The torch float64 reference of the tall cases against the numpy one, at M = 4 100: every reference and every bound agree to
    1e-12 of the tensor's largest magnitude (two float64 summation orders of at most 2 048 terms)."""
    c = FwdCase(L, 4100, p=0.1)
    s = c.run()
    a, b = c.stages(s, None), c.stages(s, "cuda")
    assert set(a) == set(b)
    for n in a:
        for i in (0, 1):
            x, y = CR._f64(a[n][i]), CR._f64(b[n][i])
            x, y = np.broadcast_to(x, a[n][0].shape), np.broadcast_to(y, a[n][0].shape)
            assert np.abs(x - y).max() <= 1e-12 * np.abs(x).max(), (n, i)
    CR.check(s, b, "device reference M=4100")


# ------------------------------------------------------------------------------------------------ forward: routing operands
def _routing_check(c, s, tag):
    t = {k: v.float().cpu().numpy() for k, v in s.items()}
    t["x_in"], t["a_in"] = c.x_in, c.a_in
    ik = CR.keep_scale(c.p)
    keeps = {}
    for site, n in (("r", D), ("h", c.NC * D), ("o", D)):
        k = CR.keep(SEEDS[site], c.keys, n, c.p) if c.p > 0 else np.ones((c.M, n), bool)
        keeps["keep_" + site] = (k * ik).astype(F32)
    ex = CR.routing_forward(t, c.rt, keeps)
    for n, v in ex.items():
        bad = np.argwhere(t[n] != v)
        assert bad.size == 0, f"{tag} {n}: {len(bad)} entries differ from the routed value, the first at (row, column) {tuple(bad[0])}"
    # the LayerNorms in between, from their stored inputs
    for x, g, b, y, st in (("x_mid", "g1", "b1", "y1", "st1"), ("x_out", "g2", "b2", "y2", "st2")):
        st_ = CR.forward_stages(dict(x_in=s[x]), dict(g1=c.w[g], b1=c.w[b]), eps=c.eps)
        CR.check({"y1": s[y], "st1": s[st]}, st_, f"{tag} {y} M={c.M} p={c.p}")
    return keeps


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("M", [1, 257, 4100, 12288, 12289, 16385])
def test_forward_routing(L, M, p):
    """Signed selection matrices as weights: every product of the chain is one exact term, so x_mid, out1, h, x_out and out2 are
    compared bit for bit at every (row, column); p = 0.5 scales by exactly 2.  Narrow form up to 12 288 rows, wide above."""
    c = FwdCase(L, M, p=p, routing=True)
    s = c.run()
    assert c.plan_["form"] == int(M > 12288)
    _routing_check(c, s, "routing")


def test_forward_mask_is_the_site_hash(L):
    """The keep mask the chain applied, recovered from its outputs, is the hash of ortk_dropout_apply at all three sites: with the
    routing operands (every hidden unit active, no update zero or absorbed by its residual row) x_mid - x_in, h and x_out - x_mid
    are non-zero exactly where the element was kept.  Also: chain_ref.keep is that hash."""
    for M, keyed in ((4100, None), (12289, "subset")):
        c = FwdCase(L, M, p=0.5, routing="mask", keyed=keyed)
        s = c.run()
        keeps = _routing_check(c, s, "mask")
        for site, n, got in (("r", D, s["x_mid"] != c.f_x.views[0].view(M, D)), ("h", c.NC * D, s["h"] != 0), ("o", D, s["x_out"] != s["x_mid"])):
            want = _keep(L, SEEDS[site], c.keys, c.Mk, n, 0.5) != 0
            assert torch.equal(got, want), f"site {site}: the applied mask is not the site's hash"
            assert np.array_equal(want.cpu().numpy(), keeps["keep_" + site] != 0), "chain_ref.keep is not ortk_dropout_apply"
            assert 0.45 < want.float().mean().item() < 0.55 or M * n < 4096


# ------------------------------------------------------------------------------------------------ the backward chain
KINDS = dict(ZX=(3, 1, 1), X=(0, 1, 1), Y=(1, 0, 1), Z=(3, 0, 0))          # nin, FFN, n2


class BwdCase:
    def __init__(self, L, M, kind, p=0.1, dresa=True, keyed=False, routing=False, NC=4):
        self.L, self.M, self.kind, self.p, self.routing = L, M, kind, p, routing
        nin, hasF, n2 = KINDS[kind]
        self.nin, self.hasF, self.n2, self.NC = nin, hasF, n2, (NC if hasF else 0)
        ff = NC * D
        g = np.random.default_rng(7 * M + 1)
        gw = np.random.default_rng(77)
        mk = lambda n, k: _bf(gw.standard_normal((n, k)) * (0.5 / np.sqrt(n)))
        w = {}
        # W[x] here is the matrix the data gradient multiplies FROM THE RIGHT: gy = ain Win, gh = dz W2, gy2 = gh W1, out2 = dz Wo
        Win, W2, W1, Wo = mk(3 * D, D), mk(D, ff), mk(ff, D), mk(D, D)
        if routing:            # the streamed (transposed) blocks are selection matrices: gh[:, 512 c + k] = c dz[:, pi_c(k)], out2 = route(dz)
            U2, self.pi2, self.c2 = CR.routing_stack(NC, 21)
            Uo, self.pio, self.co = CR.routing_unit(22)
            W2, Wo = np.ascontiguousarray(U2.T), np.ascontiguousarray(Uo.T)
        if nin: w["Win"] = Win[:nin * D]
        if hasF: w["W2"], w["W1"] = W2, W1
        if n2: w["Wo"] = Wo
        w["ga"], w["gb"] = (1 + 0.1 * gw.standard_normal(D)).astype(F32), (1 + 0.1 * gw.standard_normal(D)).astype(F32)
        w["gate_scale"] = float(CR.keep_scale(p))
        self.w = w
        # the transposed arena: block (N, K) stored (K, N); a unit's rows are the OUTPUT columns of the product
        parts, off, cur = [], {}, 0
        for n in ("Win", "W2", "W1", "Wo"):
            if n in w:
                parts.append(np.ascontiguousarray(w[n].T).reshape(-1)); off[n] = cur; cur += w[n].size
        self.f_arena = Fenced([_t(np.concatenate(parts))], torch.bfloat16)
        units = [(off["Win"] + i * D, nin * D) for i in range(nin)]
        for c in range(self.NC):
            units += [(off["W2"] + c * D * D, D), (off["W1"] + c * D, ff)]
        if n2: units.append((off["Wo"], D))
        self.units = torch.tensor(units, dtype=torch.int64).cuda()
        self.f_packed = Fenced([_nan(L.lib().ortk_chain_packed_bytes(len(units)) // 2)], torch.bfloat16)
        xa, _ = R.class_rows(M, D, M + 1)
        xb, _ = R.class_rows(M, D, M + 2)
        st = lambda x: np.stack(R.forward(x, np.ones(D), np.zeros(D))[1:], 1).astype(F32)       # the fp32 rounding of the float64 statistics
        self.f_in32 = Fenced([_t(xa), _t(xb), _t(st(xa)), _t(st(xb)), _t(g.standard_normal((M, D)).astype(F32)), _t(g.standard_normal((M, D)).astype(F32)),
                              _t(w["ga"]), _t(w["gb"])])
        hg = np.maximum(g.standard_normal((M, ff)), 0) * (g.random((M, ff)) < 0.9)
        self.f_in16 = Fenced([_t(_bf(g.standard_normal((M, 3 * D)))), _t(_bf(g.standard_normal((M, D)))), _t(_bf(hg))], torch.bfloat16)
        self.prior = (0.5 * g.standard_normal((4, D))).astype(F32)
        self.f_sum = Fenced([_t(self.prior[i]) for i in range(4)])
        self.f_o32 = Fenced([_nan(M * D), _nan(M * D)])
        self.f_o16 = Fenced([_nan(M * D), _nan(M * D), _nan(M * ff), _nan(M * D)], torch.bfloat16)
        self.dresa = dresa
        self.Mk, self.keys = M, np.arange(M)
        if keyed:
            self.Mk = M + 500
            last = CR.bplan(M)["last"]
            self.keys = np.arange(M); self.keys[M - last:] += 500 - 1; self.keys[: M // 2] = np.sort(g.permutation(M // 2 + 200)[: M // 2])
            self.keys[M // 2:M - last] += 200
            self.key_dev = torch.tensor(self.keys, dtype=torch.int32).cuda()

    def args(self):
        L, M = self.L, self.M
        xa, xb, sta, stb, dresa, dresb_ext, ga, gb = self.f_in32.views
        ain, dz0, hgate = self.f_in16.views
        dxa, dxb = self.f_o32.views
        dza, dzb, gh, out2 = self.f_o16.views
        daa, dba, dab, dbb = self.f_sum.views
        a = L.BChainArgs()
        a.w16t, a.units_dev, a.n_units = L.ptr(self.f_arena.views[0]), self.units.data_ptr(), self.units.shape[0]
        a.packed, a.packed_bytes, a.M = L.ptr(self.f_packed.views[0]), self.f_packed.views[0].numel() * 2, M
        a.nin = self.nin
        if self.nin:
            a.ain, a.ld_ain = L.ptr(ain), 3 * D                 # (nin = 1 reads the first 512 columns of the 1 536-wide rows)
            a.xa, a.sta, a.ga, a.dxa, a.daa, a.dba = L.ptr(xa), L.ptr(sta), L.ptr(ga), L.ptr(dxa), L.ptr(daa), L.ptr(dba)
            if self.dresa: a.dresa = L.ptr(dresa)
            a.mask_a, a.dza, a.seed_a = (0 if self.kind == "Z" else 1), L.ptr(dza), SEEDS["a"]
        else:
            a.dz0 = L.ptr(dz0)
        if self.hasF:
            a.NC, a.hgate, a.gh, a.gate_scale = self.NC, L.ptr(hgate), L.ptr(gh), self.w["gate_scale"]
            a.xb, a.stb, a.gb, a.dxb, a.dab, a.dbb = L.ptr(xb), L.ptr(stb), L.ptr(gb), L.ptr(dxb), L.ptr(dab), L.ptr(dbb)
            a.dresb = L.ptr(dxa) if self.nin else L.ptr(dresb_ext)          # ZX: the dxa rows this call writes
            a.mask_b, a.dzb, a.seed_b = 1, L.ptr(dzb), SEEDS["b"]
        a.n2 = self.n2
        if self.n2: a.out2 = L.ptr(out2)
        a.drop_p, a.eps = self.p, 1e-6
        if self.Mk != M: a.drop_rows = self.key_dev.data_ptr()
        return a

    def present(self):
        n = (["dxa", "daa", "dba"] + (["dza"] if self.kind != "Z" else [])) if self.nin else []
        return n + (["gh", "dxb", "dab", "dbb", "dzb"] if self.hasF else []) + (["out2"] if self.n2 else [])

    def run(self):
        L, M = self.L, self.M
        a = self.args()
        want = CR.bplan(M)
        assert L.row_bchain_plan(a) == {k: want[k] for k in ("rows_per_block", "workgroups")}
        self.f_o32.buf.fill_(float("nan")); self.f_o16.buf.fill_(float("nan")); self.f_packed.buf.fill_(float("nan"))
        for v, pr in zip(self.f_sum.views, self.prior):
            v.copy_(_t(pr))
        L.check(L.lib().ortk_row_bchain(C.byref(a), L.stream_ptr()), "ortk_row_bchain")
        torch.cuda.synchronize()
        for fb in (self.f_arena, self.f_packed, self.f_in32, self.f_in16, self.f_sum, self.f_o32, self.f_o16):
            assert fb.intact(), "a fence is broken: the backward chain wrote outside its outputs"
        dxa, dxb = self.f_o32.views
        dza, dzb, gh, out2 = self.f_o16.views
        daa, dba, dab, dbb = self.f_sum.views
        full = dict(dxa=dxa.view(M, D), dxb=dxb.view(M, D), dza=dza.view(M, D), dzb=dzb.view(M, D), gh=gh.view(M, -1), out2=out2.view(M, D),
                    daa=daa, dba=dba, dab=dab, dbb=dbb)
        s = {}
        for n, v in full.items():
            if n in self.present():
                assert torch.isfinite(v).all(), f"{n}: not every entry written, or something read past an input / a stale row"
                s[n] = v.clone()
            elif n in ("daa", "dba", "dab", "dbb"):
                assert _same(v.cpu(), _t(self.prior[("daa", "dba", "dab", "dbb").index(n)])), f"{n} is not an output of this form, and it changed"
            else:
                assert torch.isnan(v).all(), f"{n} is not an output of this form, and it was written"
        self.plan_ = want
        return s

    def stages(self, s):
        M = self.M
        xa, xb, sta, stb, dresa, dresb_ext, ga, gb = self.f_in32.views
        ain, dz0, hgate = self.f_in16.views
        t = dict(ain=ain.view(M, 3 * D)[:, :max(self.nin, 1) * D], dz0=dz0.view(M, D), xa=xa.view(M, D), xb=xb.view(M, D), hgate=hgate.view(M, -1),
                 dresa=dresa.view(M, D) if self.dresa else None, ca=self.prior[:2], cb=self.prior[2:])
        t.update(s)
        t["dresb"] = s["dxa"] if self.nin else dresb_ext.view(M, D)
        w = dict(self.w)
        if self.nin and self.kind != "Z": w["keep_a"] = _keep(self.L, SEEDS["a"], self.keys, self.Mk, D, self.p)
        if self.hasF: w["keep_b"] = _keep(self.L, SEEDS["b"], self.keys, self.Mk, D, self.p)
        return CR.backward_stages(t, w, self.plan_["workgroups"], p=self.p, device="cuda" if M > CPU_ROWS else None)

    def check(self, tag):
        s = self.run()
        st = self.stages(s)
        CR.check(s, st, f"bchain {self.kind} {tag} M={self.M} p={self.p} {self.plan_}")
        s2 = self.run()
        nb = self.plan_["workgroups"]
        for n in s:
            if n in ("daa", "dba", "dab", "dbb"):      # float atomics in any order: the rerun bound of the LayerNorm tests
                ta, tb = st["_rerun_a" if n in ("daa", "dba") else "_rerun_b"]
                r = R.ratio(np.abs(CR._f64(s[n]) - CR._f64(s2[n])), 2 * nb * CR.U * (ta if n in ("daa", "dab") else tb))
                assert r <= 1.0, (n, r)
            else:
                assert _same(s[n], s2[n]), f"{n}: a rerun changed bits"
        return s


@pytest.mark.parametrize("M", CR.BWD_ROWS)
@pytest.mark.parametrize("kind", ["ZX", "X", "Y", "Z"])
def test_backward(L, kind, M):
    """ZX = [dQKV . Wqkv -> LN' -> FFN' -> LN' -> . Wco] with dresb the dxa rows the call itself writes, X = its tail on an existing
    masked gradient, Y = [dq . Wcq -> LN' -> . Wo], Z = [dQKV . Wqkv -> LN'] without a masked copy; p = 0.1."""
    BwdCase(L, M, kind, p=0.1).check("")


@pytest.mark.parametrize("M,kind,p,dresa,keyed", [(257, "ZX", 0.0, True, False), (4100, "ZX", 0.0, True, False), (257, "ZX", 0.1, False, False),
                                                  (4100, "Y", 0.1, False, False), (257, "ZX", 0.1, True, True), (4100, "ZX", 0.1, True, True),
                                                  (8200, "Y", 0.1, True, True), (4100, "X", 0.1, True, True)])
def test_backward_forms(L, M, kind, p, dresa, keyed):
    """gate_scale 1 (p = 0), no dresa, and ortk_bchain_args.drop_rows (the partial last block keyed elsewhere than its neighbours)."""
    BwdCase(L, M, kind, p=p, dresa=dresa, keyed=keyed).check(f"dresa={int(dresa)} keyed={int(keyed)}")


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("M", [257, 4100])
def test_backward_routing(L, M, p):
    """Selection matrices as W2^T and Wo^T: gh == gate x scale x c dz[:, pi(k)] (scale exactly 1 or 2) and out2 == c dzb[:, pi(j)], bit
    for bit, from the stored dza / dzb."""
    c = BwdCase(L, M, "ZX", p=p, routing=True)
    s = c.run()
    hgate = c.f_in16.views[2].view(M, -1).float().cpu().numpy()
    gh = CR.route_stack(s["dza"].float().cpu().numpy(), c.pi2, c.c2) * F32(c.w["gate_scale"]) * (hgate > 0)
    bad = np.argwhere(s["gh"].float().cpu().numpy() != gh.astype(F32))
    assert bad.size == 0, f"gh: {len(bad)} entries differ from the routed value, the first at {tuple(bad[0])}"
    o = CR.route(s["dzb"].float().cpu().numpy(), c.pio, c.co)
    bad = np.argwhere(s["out2"].float().cpu().numpy() != o)
    assert bad.size == 0, f"out2: {len(bad)} entries differ from the routed value, the first at {tuple(bad[0])}"
    CR.check({k: v for k, v in s.items() if k not in ("gh", "out2")}, c.stages(s), f"bchain routing M={M} p={p}")
