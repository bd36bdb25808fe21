"""Exact GEMM operands: integer-valued matrices whose every product and every partial sum, in any order, is an integer below 2^24.

fp32 accumulation of such operands is exact whatever does it (an MFMA, split-K atomics, a staged epilogue), so the result does not
depend on summation order, tiling, pipelining or atomics and must equal a float64 product BIT FOR BIT: one wrong, missing, duplicated
or stale element anywhere fails torch.equal, where a maximum-error bar against the output's scale lets it through.

Operand classes (all seeded, all with exact zeros; every generator returns the LOGICAL (rows, K) matrix in float64):
  S    integers in [-4, 4]: one bf16 part.  Everything on precision = 1 (fp32- or bf16-typed operands).
  T    {-1, 0, 1} with at most 15 non-zeros per row: the partner of W3 (at most 15 non-zero products per output).
  W3   odd-ish integers of 19-20 significant bits: three round-to-nearest bf16 parts.  15 x 2^20 < 2^24.
  W2   integers of 9-10 significant bits: two bf16 parts;  W2s: the same with at most 15 non-zeros per row (its partner).
The fp32 split kernels keep the six partial products a1 b1, a1 b2, a2 b1, a1 b3, a2 b2, a3 b1 of the parts: W3 x T, T x W3 and W2 x W2s
are the pairings in which every product of two parts is among them, so those kernels are exact too.

Epilogue operands keep exactness: integer bias / residual / C0 / column sums, rowscale in {0, 0.5, 1, 2}, gate_scale a power of two,
drop_p = 0.5 (1 / (1 - p) = 2).  CASES is the table tests/test_gpu_gemm_exact.py runs on the device and tests/test_gemm_exact_host.py
checks on the CPU (bounds, parts, order independence); `plan` is the launch list ortk_gemm_plan must report for the case."""
import zlib

import torch

LIM = 2.0 ** 24
SENTINEL = -8192.0          # (exact in fp32 and bf16) what C holds outside (M, N) before and after a call
DROP_P = 0.5


def _g(seed):
    return torch.Generator().manual_seed(int(seed))


def _sparse_rows(rows, cols, nnz, g):
    """0 / 1 mask with exactly min(nnz, cols) ones per row"""
    order = torch.rand(rows, cols, generator=g).argsort(dim=1)
    return (order < min(nnz, cols)).double()


def gen_S(rows, cols, seed):
    return torch.randint(-4, 5, (rows, cols), generator=_g(seed)).double()


def gen_T(rows, cols, seed, nnz=15):
    g = _g(seed)
    sign = torch.randint(0, 2, (rows, cols), generator=g).double() * 2 - 1
    return sign * _sparse_rows(rows, cols, nnz, g)


def gen_W3(rows, cols, seed):
    g = _g(seed)
    mag = torch.randint(2 ** 18, 2 ** 20, (rows, cols), generator=g).double()
    sign = torch.randint(0, 2, (rows, cols), generator=g).double() * 2 - 1
    keep = (torch.rand(rows, cols, generator=g) >= 0.125).double()
    return mag * sign * keep


def gen_W2(rows, cols, seed, nnz=None):
    g = _g(seed)
    mag = torch.randint(257, 1024, (rows, cols), generator=g).double()
    sign = torch.randint(0, 2, (rows, cols), generator=g).double() * 2 - 1
    keep = (torch.rand(rows, cols, generator=g) >= 0.125).double()
    x = mag * sign * keep
    return x if nnz is None else x * _sparse_rows(rows, cols, nnz, g)


GEN = {"S": gen_S, "T": gen_T, "W3": gen_W3, "W2": gen_W2, "W2s": lambda r, c, s: gen_W2(r, c, s, nnz=15)}
PARTS = {"S": 1, "T": 1, "W2": 2, "W2s": 2, "W3": 3}
PAIRINGS = [("W3", "T"), ("T", "W3"), ("W2", "W2s")]


def bf16_parts(x):
    """The split of the fp32 split kernels: x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2), round to nearest even.
    Returns the three parts (fp32) and what they leave over."""
    x = x.float()
    p1 = x.bfloat16().float()
    r1 = x - p1
    p2 = r1.bfloat16().float()
    r2 = r1 - p2
    p3 = r2.bfloat16().float()
    return [p1, p2, p3], r2 - p3


def parts_needed(x):
    (p1, p2, p3), _ = bf16_parts(x)
    return torch.where(p3 != 0, 3, torch.where(p2 != 0, 2, 1))


class Case:
    """One ortk_gemm call.  layout: "nn" forward (A (M,K), B (N,K)) | "nt" data gradient (B stored (K,N)) | "tt" weight gradient (both
    k-major).  pad: elements added to lda / ldb / ldc (and ldr / ldg); off: elements the A / B / C base pointers are moved off their
    16-byte alignment.  drop: None | "plain" (index m N + n) | "keyed" (row map, stride 3, offset 1).  gate: None | "f32" | "bf16"."""

    def __init__(self, name, plan, M, N, K, layout="nn", prec=1, cls=("S", "S"), adt=0, bdt=0, cdt=0, pad=(8, 8, 8), off=(0, 0, 0),
                 bias=False, relu=False, rowscale=False, resid=False, gate=None, gate_scale=1.0, drop=None, accumulate=False, splitk=0,
                 colsum=False, ln=0, tuning=None):
        self.name, self.plan, self.M, self.N, self.K, self.layout, self.prec, self.cls = name, list(plan), M, N, K, layout, prec, cls
        self.adt, self.bdt, self.cdt, self.pad, self.off = adt, bdt, cdt, pad, off
        self.bias, self.relu, self.rowscale, self.resid, self.gate, self.gate_scale, self.drop = bias, relu, rowscale, resid, gate, gate_scale, drop
        self.accumulate, self.splitk, self.colsum, self.ln, self.tuning = accumulate, splitk, colsum, ln, dict(tuning or {})
        assert not (accumulate and (cdt or (relu and splitk > 1)))       # (ReLU of a partial sum is not the ReLU of the sum)
        self.ta, self.tb = int(layout == "tt"), int(layout in ("nt", "tt"))
        self.seed = zlib.crc32(name.encode()) & 0x7FFFFFF

    def __repr__(self):
        return self.name

    def options(self):
        o = [k for k in ("bias", "relu", "rowscale", "resid", "colsum") if getattr(self, k)]
        if self.gate: o.append(f"gate={self.gate}*{self.gate_scale:g}")
        if self.drop: o.append(f"drop={self.drop}")
        if self.accumulate: o.append(f"acc/splitk={self.splitk}")
        if self.cdt: o.append("C=bf16")
        if self.ln: o.append(f"ln_mode={self.ln}")
        if any(self.off): o.append("off=%d,%d,%d" % self.off)
        o.append("pad=%d,%d,%d" % self.pad)
        o += [f"{k}={v}" for k, v in sorted(self.tuning.items())]
        return " ".join(o)


def operands(c):
    """Every operand of the case on the CPU, float64, logical shapes."""
    M, N, K, s = c.M, c.N, c.K, c.seed
    o = {"A": GEN[c.cls[0]](M, K, s + 1), "B": GEN[c.cls[1]](N, K, s + 2)}
    g = _g(s + 3)
    ri = lambda *shape, lo=-8, hi=9: torch.randint(lo, hi, shape, generator=g).double()
    if c.bias:
        o["bias"] = ri(N)
        if not o["bias"].any(): o["bias"][0] = 3.0       # (N = 1 can draw a zero: a dropped bias would go unseen)
    if c.rowscale: o["rowscale"] = torch.tensor([0.0, 0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 4, (M,), generator=g)]
    if c.resid: o["resid"] = ri(M, N)
    if c.gate: o["gate"] = ri(M, N, lo=-2, hi=3)
    if c.accumulate: o["C0"] = ri(M, N, lo=-100, hi=101)
    if c.colsum: o["cs0"] = ri(M, lo=-100, hi=101)
    if c.drop == "keyed": o["rows"] = torch.randperm(M, generator=g).to(torch.int32)
    return o


def drop_index(c, o):
    """(M, N) int64: the dropout draw each output element takes (include/ortk.h: drop_rows, drop_row_stride, drop_row_off)"""
    m = torch.arange(c.M, dtype=torch.int64)
    if c.drop == "keyed":
        m = o["rows"].long() * 3 + 1
    return m[:, None] * c.N + torch.arange(c.N, dtype=torch.int64)[None, :]


def expected(c, o, keep=None):
    """float64 reference of the whole call: the stored C (M, N) and the column sums.  keep: (M, N) of 0 / 2, the replayed draws."""
    v = o["A"] @ o["B"].t()
    if c.bias: v = v + o["bias"][None, :]
    if c.relu: v = v.clamp_min(0)
    if c.rowscale: v = v * o["rowscale"][:, None]
    if c.drop: v = v * keep
    if c.gate: v = torch.where(o["gate"] > 0, v * c.gate_scale, torch.zeros_like(v))
    if c.resid: v = v + o["resid"]
    if c.accumulate: v = v + o["C0"]
    cs = (o["cs0"] + o["A"].sum(1)) if c.colsum else None
    return v, cs


def bound(c, o):
    """float64 magnitudes that must stay below 2^24 for the case to be exact in fp32:
      sum     |A| |B|^T max + |C0| max + |bias| max + |resid| max: no partial sum, in any order, leaves the exact integers;
      parts   the same product bound over the bf16 parts the split kernels multiply (sum_i |A_i|) (sum_j |B_j|)^T;
      stored  where a residual or C0 is added behind the epilogue's scale factors (row scale, 1 / (1 - p) = 2, gate scale): the scaled
              value's span, largest magnitude over its last bit (a factor of 0.5 moves the last bit down);
      colsum  sum_k |A| + |colsum0|."""
    prod = (o["A"].abs() @ o["B"].abs().t()).max().item()
    extra = {k: (o[k].abs().max().item() if k in o else 0.0) for k in ("C0", "bias", "resid")}
    pa, pb = (sum(q.double().abs() for q in bf16_parts(o[k])[0]) for k in ("A", "B"))
    f = ([2.0, 0.5] if c.rowscale else []) + ([2.0] if c.drop else []) + ([c.gate_scale] if c.gate else [])
    up, down = 1.0, 1.0
    for x in f:
        if x > 1: up *= x
        if x < 1: down /= x
    out = {"sum": prod + sum(extra.values()), "parts": (pa @ pb.t()).max().item() + sum(extra.values()),
           "stored": ((prod + extra["bias"]) * up + extra["resid"] + extra["C0"]) * down if (c.resid or c.accumulate) else 0.0}
    if c.colsum: out["colsum"] = (o["A"].abs().sum(1) + o["cs0"].abs()).max().item()
    return out


def _opts(i):
    return [dict(bias=True, relu=True, resid=True), dict(rowscale=True, cdt=1, bias=True), dict(gate="f32", gate_scale=0.5, resid=True),
            dict(gate="bf16", gate_scale=4.0, drop="plain", bias=True), dict(drop="keyed", relu=True, bias=True, resid=True, cdt=1), dict()][i % 6]


def _cases():
    cs = []
    DT = ("f32", "bf16")
    TT = {"nn": "0,0", "nt": "0,1", "tt": "1,1"}
    # ---- register-staged gemm_bf16_kernel: three layouts x {fp32, bf16} A x {fp32, bf16} B x guarded / fast
    tails = [(1, 127, 1), (127, 129, 31), (129, 257, 33), (257, 1, 63), (127, 127, 65), (129, 129, 70), (257, 257, 70), (1, 1, 33), (257, 127, 31),
             (129, 1, 65), (127, 257, 63), (1, 129, 1)]
    splits = [(129, 127, 70, 2), (127, 257, 200, 3), (257, 129, 520, 8), (1, 127, 130, 1), (129, 129, 65, 2), (257, 127, 330, 3), (127, 1, 1000, 8),
              (129, 257, 63, 1), (127, 129, 129, 2), (1, 257, 257, 3), (257, 257, 577, 8), (129, 1, 70, 1)]
    i = 0
    for lay in ("nn", "nt", "tt"):
        for adt in (0, 1):
            for bdt in (0, 1):
                inst = f"bf16<{TT[lay]},{DT[adt]},{DT[bdt]},"
                kw = dict(layout=lay, adt=adt, bdt=bdt)
                if not (lay == "nn" and adt and bdt):      # (forward bf16 x bf16 full tiles: the LDS-DMA kernels take them)
                    fo = [dict(bias=True, relu=True, resid=True, cdt=1), dict(gate="bf16", gate_scale=2.0, drop="keyed", bias=True),
                          dict(accumulate=True, splitk=2, bias=True, resid=True, colsum=lay == "tt"), dict(rowscale=True, gate="f32", gate_scale=0.25)][i % 4]
                    M, N, K = [(128, 256, 128), (256, 128, 64), (128, 128, 192)][i % 3]
                    cs.append(Case(f"bf16_fast_{lay}_{DT[adt]}_{DT[bdt]}", [inst + "1>"], M, N, K, **kw, **fo))
                M, N, K = tails[i]
                odd = i % 2 == 1            # unaligned base pointers and leading dimensions: the element-wise loads and stores
                cs.append(Case(f"bf16_tail_{lay}_{DT[adt]}_{DT[bdt]}", [inst + "0>"], M, N, K, **kw, pad=(3, 5, 7) if odd else (8, 8, 8),
                               off=(1, 1, 1) if odd else (0, 0, 0), colsum=(lay == "tt" and i % 3 == 0), **_opts(i)))
                M, N, K, sk = splits[i]
                so = [dict(bias=True), dict(resid=True), dict(rowscale=True), dict(gate="f32", gate_scale=2.0), dict(drop="plain"), dict()][i % 6]
                cs.append(Case(f"bf16_splitk_{lay}_{DT[adt]}_{DT[bdt]}", [inst + "0>"], M, N, K, **kw, pad=(8, 8, 8) if odd else (1, 3, 5),
                               off=(0, 0, 0) if odd else (1, 1, 1), accumulate=True, splitk=sk, colsum=lay == "tt", **so))
                i += 1
    # ---- LDS-DMA kernels (forward layout, bf16 x bf16, full column / K tiles; ragged M: the clamped last row tile)
    bb = dict(adt=1, bdt=1)
    t64off = {"gemm_t64": -1}
    cs += [
        Case("dma64_8_plain", ["bf16_dma64<8>"], 128, 128, 64, **bb),
        Case("dma64_8_ragged", ["bf16_dma64<8>"], 200, 256, 128, **bb, bias=True, relu=True, resid=True, cdt=1),
        Case("dma64_3_ragged", ["bf16_dma64<3>"], 6100, 256, 64, **bb, bias=True, resid=True),
        Case("glds_lean0", ["bf16_glds<0,0>"], 129, 128, 64, **bb, bias=True, relu=True, resid=True, cdt=1, tuning=t64off),
        Case("glds_lean1", ["bf16_glds<0,1>"], 129, 256, 128, **bb, drop="keyed", bias=True, resid=True),
        Case("glds_lean2", ["bf16_glds<0,2>"], 300, 128, 64, **bb, gate="f32", gate_scale=2.0),
        Case("glds_lean3", ["bf16_glds<0,3>"], 129, 128, 192, **bb, gate="bf16", gate_scale=0.5, drop="plain", bias=True, relu=True, resid=True, cdt=1),
        Case("glds_general_rowscale", ["bf16_glds<0,-1>"], 129, 128, 64, **bb, rowscale=True, bias=True),
        Case("glds_general_switch", ["bf16_glds<0,-1>"], 129, 256, 64, **bb, gate="bf16", gate_scale=2.0, drop="plain", cdt=1, tuning={"gemm_epilogue": 1}),
        Case("glds_general_splitk3", ["bf16_glds<0,-1>"], 256, 128, 256, **bb, accumulate=True, splitk=3, bias=True, resid=True),
        Case("glds_general_splitk8", ["bf16_glds<0,-1>"], 128, 256, 512, **bb, accumulate=True, splitk=8, rowscale=True),
        # the big tile needs at least 128 tiles of 256 x 256
        Case("dma256_lean0", ["bf16_dma256<0>"], 3900, 2048, 64, **bb, bias=True, relu=True, resid=True, cdt=1, tuning=t64off),
        Case("dma256_lean1", ["bf16_dma256<1>"], 4096, 2048, 64, **bb, drop="keyed", resid=True),
        Case("dma256_lean2", ["bf16_dma256<2>"], 3900, 2048, 64, **bb, gate="f32", gate_scale=0.5, bias=True),
        Case("dma256_lean3", ["bf16_dma256<3>"], 3900, 2048, 128, **bb, gate="bf16", gate_scale=2.0, drop="plain", bias=True, relu=True, resid=True, cdt=1),
        Case("dma256_lean3_narrow", ["bf16_dma256<3>"], 3900, 2048, 64, **bb, pad=(8, 8, 4), gate="bf16", gate_scale=2.0, drop="plain", cdt=1),
        Case("dma256_general_rowscale", ["bf16_dma256<-1>"], 3900, 2048, 64, **bb, rowscale=True, bias=True, cdt=1),
        Case("dma256_general_switch", ["bf16_dma256<-1>"], 3900, 2048, 64, **bb, drop="plain", resid=True, tuning={"gemm_epilogue": 1}),
        # 256 n + 128 columns: two launches
        Case("nsplit_lean0", ["bf16_dma256<0>", "bf16_glds<0,0>"], 3900, 2176, 64, **bb, bias=True, resid=True),
        Case("nsplit_lean1", ["bf16_dma256<1>", "bf16_glds<0,1>"], 3900, 2176, 64, **bb, drop="plain", bias=True, cdt=1),
    ]
    # ---- fp32 split kernels, forward layout: all six instances x the three pairings
    names = {2: "f32x3<1,1,2,2,2>", 3: "f32x3<2,1,2,2,3>", 4: "f32x3<2,2,2,2,3>", 5: "f32x3p<1,1,2,2,3>", 6: "f32x3p<2,1,2,2,2>", 7: "f32x3p<2,2,4,2,1>"}
    i = 0
    for v in range(2, 8):
        for pa in PAIRINGS:
            M, N, K = (300, 200, 96) if v == 7 else (130, 70, 96)
            fo = [dict(bias=True, relu=True, resid=True), dict(), dict(rowscale=True, bias=True), dict(gate="f32", gate_scale=2.0, drop="plain")][i % 4]
            cs.append(Case(f"f32x3_split{v}_{pa[0]}x{pa[1]}", [names[v]], M, N, K, prec=0, cls=pa, pad=(4, 8, 4), tuning={"f32_split": v}, **fo))
            i += 1
    # ---- fp32 split kernels, k-major layouts; the fp32 MFMA kernel in all three layouts
    for pa in PAIRINGS:
        tag = f"{pa[0]}x{pa[1]}"
        cs_ok = pa[0] != "W3"        # (column sums of a dense W3 operand leave the exact integers)
        cs += [
            Case(f"f32x3t_dgrad_{tag}", ["f32x3t<0,0>"], 130, 72, 96, layout="nt", prec=0, cls=pa, pad=(4, 4, 3), bias=True, relu=True, resid=True),
            Case(f"f32x3t_wgrad_{tag}", ["f32x3t<1,0>"], 132, 72, 70, layout="tt", prec=0, cls=pa, pad=(4, 8, 1), colsum=cs_ok),
            Case(f"f32x3t_wgrad_acc_{tag}", ["f32x3t<1,1>"], 132, 72, 200, layout="tt", prec=0, cls=pa, pad=(4, 4, 4), accumulate=True, splitk=3, colsum=cs_ok),
            Case(f"f32_nn_{tag}", ["f32<0,0>"], 129, 70, 33, prec=0, cls=pa, pad=(3, 1, 5), off=(1, 0, 1), bias=True, relu=True, resid=True),
            Case(f"f32_nn_nosplit_{tag}", ["f32<0,0>"], 130, 129, 64, prec=0, cls=pa, gate="f32", gate_scale=2.0, drop="keyed", tuning={"f32_split": 0}),
            Case(f"f32_nt_{tag}", ["f32<0,1>"], 129, 70, 65, layout="nt", prec=0, cls=pa, pad=(1, 3, 8), rowscale=True, bias=True),
            Case(f"f32_tt_{tag}", ["f32<1,1>"], 70, 129, 130, layout="tt", prec=0, cls=pa, pad=(3, 3, 3), off=(0, 1, 0), resid=True),
            Case(f"f32_tt_acc_{tag}", ["f32<1,1>"], 132, 72, 200, layout="tt", prec=0, cls=pa, accumulate=True, splitk=3, tuning={"f32_split": 0}),
        ]
        if cs_ok:
            cs.append(Case(f"f32_tt_colsum_{tag}", ["colsum", "f32<1,1>"], 129, 70, 131, layout="tt", prec=0, cls=pa, pad=(1, 2, 3), colsum=True,
                           accumulate=True, splitk=2, bias=True))
    # ---- LayerNorm forward fused into the epilogue: the stored C (product + bias + residual) is exact; and the separate-kernels form
    cs += [
        Case("ln_fwd_fused", ["bf16_row512"], 129, 512, 128, **bb, pad=(8, 8, 0), bias=True, resid=True, drop="plain", ln=1),
        Case("ln_fwd_separate", ["bf16<0,0,f32,f32,0>", "layernorm_fwd"], 50, 96, 80, pad=(8, 8, 0), bias=True, resid=True, ln=1),
    ]
    assert len({c.name for c in cs}) == len(cs)
    return cs


CASES = _cases()

# Every kernel instance ortk_gemm.hip can launch (ortk_gemm_plan's names), except:
#   bf16_glds<0,4>, bf16_glds<0,5>      the soft-max-statistics / sampling epilogues (tile_stats, tile_samp): their outputs are not exact
#                                       (test_gemm_tile_softmax_partials, test_gemm_gumbel_max_candidates hold them)
#   bf16_rowln_bwd<2..5>, layernorm_bwd_drop_rows     the LayerNorm-backward panels (ln_mode 2): not exact (test_gemm_with_fused_layernorm_backward)
#   bf16_glds<1,-1>                     unreachable: plan_dma takes it for K % 64 == 32, but bf16_fast_nk, which plan_dma requires first,
#                                       holds for K % 64 == 0 only
#   bf16<0,0,bf16,bf16,1>               forward bf16 x bf16 with full tiles is always an LDS-DMA launch; the register-staged instance is left
#                                       for column counts above 128 x 65 535 (the 16-bit column-tile argument), which no test can hold
INSTANCES = sorted(
    [f"bf16<{t},{a},{b},{f}>" for t in ("0,0", "0,1", "1,1") for a in ("f32", "bf16") for b in ("f32", "bf16") for f in (0, 1)
     if (t, a, b, f) != ("0,0", "bf16", "bf16", 1)] +
    ["bf16_dma64<8>", "bf16_dma64<3>", "bf16_glds<0,0>", "bf16_glds<0,1>", "bf16_glds<0,2>", "bf16_glds<0,3>", "bf16_glds<0,-1>",
     "bf16_dma256<0>", "bf16_dma256<1>", "bf16_dma256<2>", "bf16_dma256<3>", "bf16_dma256<-1>", "bf16_row512",
     "f32x3<1,1,2,2,2>", "f32x3<2,1,2,2,3>", "f32x3<2,2,2,2,3>", "f32x3p<1,1,2,2,3>", "f32x3p<2,1,2,2,2>", "f32x3p<2,2,4,2,1>",
     "f32x3t<0,0>", "f32x3t<1,0>", "f32x3t<1,1>", "f32<0,0>", "f32<0,1>", "f32<1,1>", "colsum", "layernorm_fwd"])
EXCLUDED = ["bf16_glds<0,4>", "bf16_glds<0,5>", "bf16_rowln_bwd<2>", "bf16_rowln_bwd<3>", "bf16_rowln_bwd<4>", "bf16_rowln_bwd<5>",
            "layernorm_bwd_drop_rows", "bf16_glds<1,-1>", "bf16<0,0,bf16,bf16,1>"]


def lds(c):
    """leading dimensions (elements) of A, B, C as stored"""
    a = (c.M if c.ta else c.K) + c.pad[0]
    b = (c.N if c.tb else c.K) + c.pad[1]
    return a, b, c.N + c.pad[2]


def fill_args(c, a, ptr, have):
    """Set every scalar field of a GemmArgs for the case; ptr: name -> address for A, B, C and the optional operands in `have`."""
    a.A, a.B, a.C = ptr["A"], ptr["B"], ptr["C"]
    a.lda, a.ldb, a.ldc = lds(c)
    a.M, a.N, a.K, a.transA, a.transB, a.precision = c.M, c.N, c.K, c.ta, c.tb, c.prec
    a.a_dtype, a.b_dtype, a.c_dtype = c.adt, c.bdt, c.cdt
    a.relu, a.accumulate, a.splitk = int(c.relu), int(c.accumulate), c.splitk
    for k in ("bias", "rowscale", "resid", "gate", "colsum"):
        if k in have: setattr(a, k, ptr[k])
    if c.resid: a.ldr = c.N + c.pad[2]
    if c.gate: a.ldg, a.gate_dtype, a.gate_scale = c.N + c.pad[2], int(c.gate == "bf16"), c.gate_scale
    if c.drop:
        a.drop_p, a.drop_seed = DROP_P, 1000 + c.seed % 1000
        if c.drop == "keyed": a.drop_rows, a.drop_row_stride, a.drop_row_off = ptr["rows"], 3, 1
    if c.ln:
        a.ln_mode, a.ln_y_dtype, a.ln_eps = c.ln, 1, 1e-6
        a.ln_a, a.ln_b, a.ln_y, a.ln_stats = ptr["ln_a"], ptr["ln_b"], ptr["ln_y"], ptr["ln_stats"]
    return a


def fake_args(c, a):
    """GemmArgs of the case over made-up addresses with the case's alignment: ortk_gemm_plan tests pointers for alignment only."""
    esz = {"A": 2 if c.adt else 4, "B": 2 if c.bdt else 4, "C": 2 if c.cdt else 4}
    ptr = {k: 0x1000000 * (i + 1) + c.off[i] * esz[k] for i, k in enumerate(("A", "B", "C"))}
    have = [k for k in ("bias", "rowscale", "resid", "gate", "colsum") if getattr(c, k)]
    for i, k in enumerate(have + ["rows", "ln_a", "ln_b", "ln_y", "ln_stats"]):
        ptr[k] = 0x1000000 * (i + 8)
    return fill_args(c, a, ptr, have)
