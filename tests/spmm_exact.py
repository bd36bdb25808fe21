"""Exact sparse products: the case table of tests/test_gpu_spmm_exact.py (device) and tests/test_spmm_exact_host.py (CPU).

All three formats accumulate exact products in fp32 (ELL32: fmaf, ELL16: v_dot2c on bf16 pairs, GU16: the bf16 MFMA), so the method of
tests/gemm_exact.py carries over: integer operands whose partial sums stay below 2^24 give a result that does not depend on chunk
order, lane assignment, row tile or group split and must equal a float64 reference of the whole epilogue BIT FOR BIT.

A case is ONE PLAN OF SEVERAL BLOCKS plus ONE ortk_spmm call on one of them (almost always not block 0: chunk0 / slot0 / row0 /
stream_offset and the per-block step bound are then non-zero).  Operand classes (gemm_exact's generators): S x S everywhere; ELL32 also
W2 weights (9-10 significant bits) against S activations and the reverse, which a path that rounded fp32 operands to bf16 fails.
`form` is the string ortk_spmm_plan must report, `steps` (GU16) the unrolled step class the block's bound must select."""
import zlib

import torch

from gemm_exact import DROP_P, LIM, SENTINEL, gen_S, gen_W2, _g

ELL32, ELL16, GU16 = 0, 1, 2
FMT = {ELL32: "ell32", ELL16: "ell16", GU16: "gu"}
RB = {ELL32: 8, ELL16: 16}             # rows per workgroup of the ELL kernels
ZEROS = {"b50": 0.5, "b80": 0.8, "b90": 0.9, "b95": 0.95, "b975": 0.975, "b99": 0.99}


class B:
    """One block of a plan: (N outputs, K inputs) under a density pattern, stored with leading dimension K + pad, `gap` elements behind
    the previous block's end.  Patterns: b50 .. b99 Bernoulli with that share of zeros | zero | dense | onerow (one dense output among
    empty ones) | emptytail (b80 on the first 5/8 of the outputs, nothing behind) | negzero (b90, half of the zeros stored as -0.0) |
    tiny (b90, half of the zeros stored as 1e-42: non-zero in fp32, zero as bf16 — bf16 formats only)."""

    def __init__(self, N, K, pat, pad=0, gap=0):
        self.N, self.K, self.pat, self.pad, self.gap = N, K, pat, pad, gap


def gen_block(b, cls, seed):
    """(logical float64 weights, fp32 source values): they differ where the source holds -0.0 or a value below bf16's range."""
    base = {"S": gen_S, "W2": gen_W2}[cls](b.N, b.K, seed)
    full = torch.where(base == 0, torch.ones_like(base), base)
    g = _g(seed + 7)
    u = torch.rand(b.N, b.K, generator=g)
    pat = b.pat
    if pat in ZEROS: W = base * (u >= ZEROS[pat])
    elif pat == "zero": W = torch.zeros_like(base)
    elif pat == "dense": W = full
    elif pat == "onerow":
        W = torch.zeros_like(base); W[b.N // 3] = full[b.N // 3]
    elif pat == "emptytail":
        W = base * (u >= 0.8); W[b.N * 5 // 8:] = 0
    else:
        assert pat in ("negzero", "tiny"), pat
        W = base * (u >= 0.9)
    src = W.float()
    if pat in ("negzero", "tiny"):
        odd = (W == 0) & (torch.rand(b.N, b.K, generator=g) < 0.5)
        src[odd] = -0.0 if pat == "negzero" else 1e-42
        assert odd.any()
    return W, src


class Case:
    """fmt: plan format; blocks: the plan; call: the block the product runs on; xdt / ydt / wdt: dtypes (0 fp32, 1 bf16) of X, Y and the
    weight source; cls: (weight class, activation class); pad: elements added to ldx, ldy, ldr, ldg; off: elements the X base, the Y base
    and the epilogue operands (bias, rowscale, residual, gate) are moved off their 16-byte alignment.
    drop: None | "plain" (index m N + n) | "keyed" (drop_rows, a permutation).  gate: None | "f32" | "bf16"."""

    def __init__(self, name, fmt, blocks, M, form, call=1, steps=None, xdt=None, ydt=0, wdt=0, cls=("S", "S"), pad=(8, 4, 4, 4), off=(0, 0, 0),
                 bias=False, relu=False, rowscale=False, resid=False, gate=None, gate_scale=1.0, drop=None, tuning=None):
        self.name, self.fmt, self.blocks, self.M, self.form, self.call, self.steps = name, fmt, list(blocks), M, form, call, steps
        self.xdt = (0 if fmt == ELL32 else 1) if xdt is None else xdt
        self.ydt, self.wdt, self.cls, self.pad, self.off = ydt, wdt, cls, pad, off
        self.bias, self.relu, self.rowscale, self.resid, self.gate, self.gate_scale, self.drop = bias, relu, rowscale, resid, gate, gate_scale, drop
        self.tuning = dict(tuning or {})
        self.accumulate = self.colsum = False          # (gemm_exact.expected reads them)
        self.N, self.K = self.blocks[call].N, self.blocks[call].K
        self.seed = zlib.crc32(name.encode()) & 0x7FFFFFF
        assert (steps is not None) == (fmt == GU16)
        assert fmt == ELL32 or cls == ("S", "S")        # the bf16 formats hold one bf16 part
        assert fmt != ELL32 or all(b.pat != "tiny" for b in blocks)
        assert not (wdt and any(b.pat == "tiny" for b in blocks))

    def __repr__(self):
        return self.name

    def options(self):
        o = [k for k in ("bias", "relu", "rowscale", "resid") if getattr(self, k)]
        if self.gate: o.append(f"gate={self.gate}*{self.gate_scale:g}")
        if self.drop: o.append(f"drop={self.drop}")
        o.append("X=%s Y=%s W=%s" % tuple("f32" if d == 0 else "bf16" for d in (self.xdt, self.ydt, self.wdt)))
        if any(self.off): o.append("off=%d,%d,%d" % self.off)
        o.append("pad=%d,%d,%d,%d" % self.pad)
        o += [f"{k}={v}" for k, v in sorted(self.tuning.items())]
        return " ".join(o)

    def shapes(self):
        return "M %5d blocks %s call %d" % (self.M, "+".join("%dx%d:%s" % (b.N, b.K, b.pat) for b in self.blocks), self.call)


def layout(c):
    """Where the blocks lie in the weight source: [(element offset, ld)], and the source's length."""
    at, out = 0, []
    for b in c.blocks:
        at += b.gap
        out.append((at, b.K + b.pad))
        at += b.N * (b.K + b.pad)
    return out, at


def capacity(c, b, src):
    """ELL entries reserved for a block: its chunks padded to their longest member and the entry granule, whatever the order
    (counted on the source values: a value below bf16's range takes an entry, -0.0 does not)."""
    gran = 8 if c.fmt == ELL16 else 4
    longest = int((src != 0).sum(1).max())
    return ((longest + gran - 1) // gran * gran) * 64 * ((b.N + 63) // 64)


def block_dicts(c, o):
    """The plan as sparse.SparsePlan takes it"""
    lay, _ = layout(c)
    return [dict(offset=at, N=b.N, K=b.K, ld=ld, capacity=capacity(c, b, src)) for b, (at, ld), src in zip(c.blocks, lay, o["Wsrc"])]


def operands(c):
    """Every operand of the case on the CPU: "W" / "Wsrc" lists over the blocks, "A" the activations (M, K), "B" the called block."""
    s = c.seed
    ws = [gen_block(b, c.cls[0], s + 11 * i) for i, b in enumerate(c.blocks)]
    o = {"W": [w for w, _ in ws], "Wsrc": [x for _, x in ws]}
    o["A"] = {"S": gen_S, "W2": gen_W2}[c.cls[1]](c.M, c.K, s + 1)
    o["B"] = o["W"][c.call]
    g = _g(s + 3)
    ri = lambda *shape, lo=-8, hi=9: torch.randint(lo, hi, shape, generator=g).double()
    if c.bias:
        o["bias"] = ri(c.N)
        if not o["bias"].any(): o["bias"][0] = 3.0
    if c.rowscale: o["rowscale"] = torch.tensor([0.0, 0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 4, (c.M,), generator=g)]
    if c.resid: o["resid"] = ri(c.M, c.N)
    if c.gate: o["gate"] = ri(c.M, c.N, lo=-2, hi=3)
    if c.drop == "keyed": o["rows"] = torch.randperm(c.M, generator=g).to(torch.int32)
    return o


def drop_index(c, o):
    """(M, N) int64: the dropout draw of each output element: (drop_rows ? drop_rows[m] : m) N + n  (include/ortk.h)"""
    m = o["rows"].long() if c.drop == "keyed" else torch.arange(c.M, dtype=torch.int64)
    return m[:, None] * c.N + torch.arange(c.N, dtype=torch.int64)[None, :]


def bound(c, o):
    """float64 magnitudes that must stay below 2^24 (gemm_exact.bound): `sum` the largest row sum of |x| |w| plus the bias and the
    residual; `stored` where a residual is added behind the epilogue's scale factors, the scaled value's span over its last bit."""
    prod = (o["A"].abs() @ o["B"].abs().t()).max().item() if c.K else 0.0
    extra = {k: (o[k].abs().max().item() if k in o else 0.0) for k in ("bias", "resid")}
    f = ([2.0, 0.5] if c.rowscale else []) + ([2.0] if c.drop else []) + ([c.gate_scale] if c.gate else [])
    up, down = 1.0, 1.0
    for x in f:
        if x > 1: up *= x
        if x < 1: down /= x
    return {"sum": prod + sum(extra.values()), "stored": ((prod + extra["bias"]) * up + extra["resid"]) * down if c.resid else 0.0}


def gu_bound(W):
    """The GU16 builder's per-block step bound for weights W (N, K): over the groups of 16 outputs, the chunks of 512 inputs and the 8
    residue classes k mod 8, the largest number of input columns in which any output of the group is non-zero, in k-steps of 4."""
    N, K = W.shape
    nz = (W != 0).numpy()
    best = 0
    for g0 in range(0, N, 16):
        u = nz[g0:g0 + 16].any(0)
        for k0 in range(0, K, 512):
            ch = u[k0:k0 + 512]
            for r in range(8):
                best = max(best, int(ch[r::8].sum()))
    return (best + 3) // 4


def step_class(bound_):
    return 8 if bound_ <= 8 else 12 if bound_ <= 12 else 16


LEAN = dict(bias=True, relu=True, resid=True)


def _ell_cases(e):
    T, R = ("f32", "bf16")[e], RB[e]
    sf = "fast" if e == ELL16 else "slow"          # the staging of a bf16 X with K % 8 == 0, padded ldx, aligned base
    n = FMT[e]
    F = lambda inst, rpw, stage, epi: f"ell<{T},{inst}>:rpw={rpw}:stage={stage}:epi={epi}"
    two = lambda N, K, pat, **kw: [B(70, 40, "b80"), B(N, K, pat, **kw)]
    cs = [
        # ---- the instances: KT x NT x ALIAS, row tails around the row tile
        Case(f"{n}_k512_nt512_above", e, two(132, 72, "b80", pad=8, gap=8), R + 1, F("512,512,0", 1, sf, "lean"), **LEAN),
        Case(f"{n}_one_row", e, [B(64, 24, "dense"), B(5, 3, "b50", pad=1, gap=3)], 1, F("512,512,0", 1, "slow", "general"), bias=True, ydt=1),
        Case(f"{n}_k512_nt256", e, [B(64, 72, "zero"), B(1100, 72, "b95")], 220 * R, F("512,256,0", 1, sf, "general"), gate="f32", gate_scale=2.0, resid=True),
        Case(f"{n}_k2048_alias_below", e, [B(200, 520, "b90"), B(132, 520, "b975", pad=8, gap=8)], R - 1, F("2048,512,1", 1, sf, "lean"), ydt=1, **LEAN),
        Case(f"{n}_k2048_alias_off", e, two(132, 520, "onerow"), R, F("2048,512,0", 1, sf, "general"), drop="plain", bias=True, tuning={"spmm_alias": 0}),
        Case(f"{n}_k2048_alias_nt256", e, [B(64, 40, "b50"), B(1100, 520, "b99")], 220 * R + 1, F("2048,256,1", 1, sf, "general"), rowscale=True, bias=True),
        Case(f"{n}_ffn_dgrad_block0", e, [B(512, 2048, "b95"), B(64, 40, "zero")], R + 1, F("2048,512,1", 1, sf, "lean"), call=0, wdt=1, **LEAN),
        Case(f"{n}_dense_block", e, [B(64, 40, "b50"), B(70, 512, "dense")], R, F("512,512,0", 1, sf, "general"), gate="bf16", gate_scale=0.5, pad=(8, 4, 4, 3)),
        # ---- ranges per workgroup: 2 and 3 capped by the block's ranges, 4, and 5 ranges in groups of 4
        Case(f"{n}_rpw2", e, [B(64, 40, "b80"), B(600, 72, "emptytail")], 1025 * R, F("512,256,0", 2, sf, "lean"), **LEAN),
        Case(f"{n}_rpw3", e, [B(64, 40, "b80"), B(1100, 72, "b90")], 683 * R - 3, F("512,256,0", 3, sf, "lean"), bias=True, relu=True),
        Case(f"{n}_rpw4", e, [B(64, 40, "b80"), B(1600, 520, "b975")], 513 * R, F("2048,512,0", 4, sf, "lean"), resid=True),
        Case(f"{n}_rpw4_of_5", e, [B(64, 40, "b80"), B(2100, 520, "b99")], 410 * R, F("2048,256,0", 4, sf, "lean"), bias=True, ydt=1),
        # ---- the slow staging, reason by reason
        Case(f"{n}_stage_k70", e, two(132, 70, "negzero", pad=2), R + 1, F("512,512,0", 1, "slow", "lean"), **LEAN),
        Case(f"{n}_stage_ldx", e, two(132, 72, "negzero", gap=3), R + 1, F("512,512,0", 1, "slow", "lean"), pad=(3, 4, 4, 4), wdt=1, **LEAN),
        Case(f"{n}_stage_base", e, two(132, 520, "b90"), R + 1, F("2048,512,1", 1, "slow", "lean"), off=(2, 0, 0), **LEAN),
        Case(f"{n}_stage_other_x", e, two(132, 72, "b80"), R + 1, F("512,512,0", 1, "slow", "lean"), xdt=1 - (0 if e == ELL32 else 1), **LEAN),
        # ---- the general epilogue, reason by reason (each lean but for one thing), and its scalar tails
        Case(f"{n}_epi_ldy", e, two(132, 72, "b80"), R + 1, F("512,512,0", 1, sf, "general"), pad=(8, 3, 4, 4), **LEAN),
        Case(f"{n}_epi_ybase", e, two(132, 72, "b80"), R + 1, F("512,512,0", 1, sf, "general"), off=(0, 1, 0), ydt=1, **LEAN),
        Case(f"{n}_epi_operands", e, two(132, 72, "b80"), R + 1, F("512,512,0", 1, sf, "general"), off=(0, 0, 1), **LEAN),
        Case(f"{n}_epi_ldr", e, two(132, 520, "b90"), R + 1, F("2048,512,1", 1, sf, "general"), pad=(8, 4, 5, 4), **LEAN),
        Case(f"{n}_epi_n70_keyed", e, two(70, 72, "b80"), 2 * R + 1, F("512,512,0", 1, sf, "general"), drop="keyed", gate="bf16", gate_scale=4.0,
             pad=(8, 1, 3, 5), bias=True, relu=True, resid=True, rowscale=True),
    ]
    if e == ELL16:
        cs.append(Case(f"{n}_tiny_weights", e, two(132, 72, "tiny"), R + 1, F("512,512,0", 1, "fast", "lean"), **LEAN))
    else:       # fp32 operands keep all their bits
        cs += [Case(f"{n}_w2_weights", e, two(132, 520, "b90"), R + 1, F("2048,512,1", 1, "slow", "lean"), cls=("W2", "S"), **LEAN),
               Case(f"{n}_w2_activations", e, two(132, 72, "b80"), R + 1, F("512,512,0", 1, "slow", "general"), cls=("S", "W2"), rowscale=True),
               Case(f"{n}_w2_weights_2048", e, two(70, 2048, "b95"), 3, F("2048,512,1", 1, "slow", "general"), cls=("W2", "S"), bias=True)]
    return cs


def _gu_cases():
    e = GU16
    F = lambda inst, gs, stage, epi: f"gu<{inst}>:gsplit={gs}:stage={stage}:epi={epi}"
    two = lambda N, K, pat, **kw: [B(48, 72, "b80"), B(N, K, pat, **kw)]
    return [
        # ---- the instances MT x MULTI with the row tails of each tile
        Case("gu_mt1_above", e, two(132, 72, "b80", pad=8, gap=8), 17, F("1,0", 16, "fast", "lean"), steps=8, **LEAN),
        Case("gu_mt1_below", e, two(132, 72, "b80", pad=8, gap=8), 15, F("1,0", 16, "fast", "general"), steps=8, rowscale=True),
        Case("gu_one_row", e, [B(16, 512, "dense"), B(5, 3, "b50", pad=1, gap=3)], 1, F("1,0", 8, "slow", "general"), steps=8, bias=True, ydt=1),
        Case("gu_dense_block", e, [B(5, 3, "b50"), B(32, 512, "dense")], 16, F("1,0", 8, "fast", "lean"), steps=16, **LEAN),
        Case("gu_mt1_multi", e, two(48, 520, "b90"), 33, F("1,1", 8, "fast", "lean"), steps=16, **LEAN),
        Case("gu_mt2_at", e, two(48, 520, "b90"), 2048, F("2,1", 8, "fast", "general"), steps=16, gate="f32", gate_scale=2.0, resid=True),
        Case("gu_mt2_below", e, two(132, 72, "b80"), 2079, F("2,0", 16, "fast", "lean"), steps=8, ydt=1, **LEAN),
        Case("gu_mt2_above", e, two(70, 72, "onerow"), 2081, F("2,0", 8, "fast", "general"), steps=8, bias=True),
        Case("gu_mt4_at", e, two(132, 72, "emptytail"), 8192, F("4,0", 16, "fast", "lean"), steps=8, **LEAN),
        Case("gu_mt4_below", e, two(48, 72, "b80"), 8255, F("4,0", 8, "fast", "general"), steps=8, drop="plain", bias=True),
        Case("gu_mt4_multi_above", e, two(48, 1030, "b90"), 8257, F("4,1", 8, "fast+tail", "lean"), steps=16, pad=(2, 4, 4, 4), bias=True, ydt=1),
        # ---- the data gradient of the FFN (K = 2 048, N = 512), block 0 of its plan; the step classes; the group splits
        Case("gu_ffn_dgrad_block0", e, [B(512, 2048, "b95"), B(16, 8, "zero")], 17, F("1,1", 8, "fast", "lean"), steps=12, call=0, wdt=1, **LEAN),
        Case("gu_steps8_b99", e, two(512, 512, "b99"), 17, F("1,0", 8, "fast", "lean"), steps=8, **LEAN),
        Case("gu_steps12_b95", e, two(64, 512, "b95"), 17, F("1,0", 8, "fast", "lean"), steps=12, **LEAN),
        Case("gu_steps16_b80", e, [B(64, 512, "b99"), B(64, 512, "b80")], 17, F("1,0", 8, "fast", "lean"), steps=16, **LEAN),
        Case("gu_steps8_after_dense", e, [B(64, 512, "dense"), B(64, 512, "b975")], 17, F("1,0", 8, "fast", "lean"), steps=8, **LEAN),
        Case("gu_zero_block", e, [B(64, 512, "b50"), B(64, 512, "zero")], 17, F("1,0", 8, "fast", "lean"), steps=8, **LEAN),
        Case("gu_split2_ragged", e, two(300, 72, "b80"), 33, F("1,0", 16, "fast", "lean"), steps=8, **LEAN),
        Case("gu_split4", e, two(512, 72, "b90"), 33, F("1,0", 8, "fast", "lean"), steps=8, **LEAN),
        Case("gu_split8_ragged", e, two(1100, 512, "b975"), 33, F("1,0", 16, "fast", "lean"), steps=8, resid=True),
        Case("gu_split16", e, two(2048, 72, "b90"), 33, F("1,0", 8, "fast", "lean"), steps=8, bias=True),
        Case("gu_split1_long_grid", e, two(512, 72, "b90"), 24576, F("4,0", 32, "fast", "lean"), steps=8, ydt=1, bias=True),
        # ---- the slow staging, reason by reason; ragged chunks
        Case("gu_stage_f32_x", e, two(132, 72, "negzero"), 17, F("1,0", 16, "slow", "lean"), steps=8, xdt=0, **LEAN),
        Case("gu_stage_ldx", e, two(132, 520, "tiny"), 17, F("1,1", 16, "slow", "lean"), steps=16, pad=(3, 4, 4, 4), **LEAN),
        Case("gu_stage_base", e, two(132, 72, "negzero", gap=3), 17, F("1,0", 16, "slow", "lean"), steps=8, off=(2, 0, 0), wdt=1, **LEAN),
        Case("gu_stage_k70", e, two(132, 70, "b80", pad=2), 17, F("1,0", 16, "slow", "lean"), steps=8, **LEAN),
        Case("gu_stage_k1030", e, two(48, 1030, "b80", pad=2), 17, F("1,1", 8, "fast+tail", "lean"), steps=16, pad=(2, 4, 4, 4), **LEAN),
        Case("gu_stage_k1030_f32_x", e, two(48, 1030, "b80", pad=3, gap=1), 17, F("1,1", 8, "slow", "lean"), steps=16, xdt=0, wdt=1, **LEAN),
        # ---- the general epilogue, reason by reason, and its scalar tails
        Case("gu_epi_ldy", e, two(132, 72, "b80"), 17, F("1,0", 16, "fast", "general"), steps=8, pad=(8, 3, 4, 4), **LEAN),
        Case("gu_epi_ybase", e, two(132, 72, "b80"), 17, F("1,0", 16, "fast", "general"), steps=8, off=(0, 1, 0), ydt=1, **LEAN),
        Case("gu_epi_operands", e, two(132, 72, "b80"), 17, F("1,0", 16, "fast", "general"), steps=8, off=(0, 0, 1), **LEAN),
        Case("gu_epi_ldr", e, two(132, 520, "b90"), 17, F("1,1", 16, "fast", "general"), steps=16, pad=(8, 4, 5, 4), **LEAN),
        Case("gu_epi_n70_keyed", e, two(70, 72, "b80"), 33, F("1,0", 8, "fast", "general"), steps=8, drop="keyed", gate="bf16", gate_scale=4.0,
             pad=(8, 1, 3, 5), bias=True, relu=True, resid=True, rowscale=True),
        Case("gu_epi_gate_f32_multi", e, two(70, 520, "b90"), 2081, F("2,1", 8, "fast", "general"), steps=16, gate="f32", gate_scale=0.5, drop="plain",
             pad=(8, 2, 4, 2), ydt=1),
    ]


CASES = _ell_cases(ELL32) + _ell_cases(ELL16) + _gu_cases()
assert len({c.name for c in CASES}) == len(CASES)


def features(c, form=None):
    """What a case's plan string (and step class) adds to the coverage: the kernel instance, and per format rpw / the step class, the
    staging path and the epilogue."""
    form = c.form if form is None else form
    inst, *rest = form.split(":")
    f = FMT[c.fmt]
    out = {inst} | {f"{f}:{r}" for r in rest if not r.startswith("gsplit=")}
    if c.fmt == GU16:
        out.add(f"gu:steps={c.steps}")
    return out


# Everything the table must reach: the 18 kernel instances ortk_spmm can launch, every rpw of the ELL formats, every step class of GU16,
# every staging path and both epilogues of each format.  Excluded, with the reason:
#   ell<f32|bf16,512,512|256,1>   instantiated beside the others but unreachable: ALIAS is chosen for K > 512 only (spmm_form: the held
#                                 output tile measured no faster with 16 KB planes)
FORMS = sorted(
    [f"ell<{t},{k},{nt},{a}>" for t in ("f32", "bf16") for k in (512, 2048) for nt in (512, 256) for a in (0, 1) if not (k == 512 and a)] +
    [f"gu<{mt},{mu}>" for mt in (1, 2, 4) for mu in (0, 1)] +
    [f"{f}:rpw={r}" for f in ("ell32", "ell16") for r in (1, 2, 3, 4)] +
    ["ell32:stage=slow", "ell16:stage=fast", "ell16:stage=slow", "gu:stage=fast", "gu:stage=slow", "gu:stage=fast+tail"] +
    [f"{f}:epi={x}" for f in ("ell32", "ell16", "gu") for x in ("lean", "general")] +
    ["gu:steps=8", "gu:steps=12", "gu:steps=16"])
EXCLUDED = [f"ell<{t},512,{nt},1>" for t in ("f32", "bf16") for nt in (512, 256)]


def lds(c):
    """ldx, ldy, ldr, ldg (elements)"""
    return c.K + c.pad[0], c.N + c.pad[1], c.N + c.pad[2], c.N + c.pad[3]


def fill_args(c, a, ptr):
    """Set every field of a SpmmArgs for the case; ptr: name -> address of X, Y and the optional operands the case has."""
    a.X, a.Y = ptr["X"], ptr["Y"]
    a.ldx, a.ldy, ldr, ldg = lds(c)
    a.M, a.x_dtype, a.y_dtype, a.relu = c.M, c.xdt, c.ydt, int(c.relu)
    if c.bias: a.bias = ptr["bias"]
    if c.rowscale: a.rowscale = ptr["rowscale"]
    if c.resid: a.resid, a.ldr = ptr["resid"], ldr
    if c.gate: a.gate, a.ldg, a.gate_dtype, a.gate_scale = ptr["gate"], ldg, int(c.gate == "bf16"), c.gate_scale
    if c.drop:
        a.drop_p, a.drop_seed = DROP_P, 1000 + c.seed % 1000
        if c.drop == "keyed": a.drop_rows = ptr["rows"]
    return a


def fake_args(c, a):
    """SpmmArgs of the case over made-up addresses with the case's alignment: ortk_spmm_plan tests pointers for alignment only."""
    ptr = {"X": 0x1000000 + c.off[0] * (2 if c.xdt else 4), "Y": 0x2000000 + c.off[1] * (2 if c.ydt else 4), "rows": 0x7000000}
    for i, k in enumerate(("bias", "rowscale", "resid", "gate")):
        ptr[k] = 0x1000000 * (i + 3) + c.off[2] * (2 if (k == "gate" and c.gate == "bf16") else 4)
    return fill_args(c, a, ptr)


def fake_plan(L, fmt, blocks):
    """An ortk_sparse_plan over made-up buffer addresses for blocks given as (N, K): ortk_spmm_plan reads blocks_host only.
    Returns (the struct, the block table it points to: keep both alive)."""
    import ctypes as C
    host = (L.EllBlock * len(blocks))()
    rows = chunks = slots = 0
    for h, (N, K) in zip(host, blocks):
        h.src_offset, h.ld, h.N, h.K = 0, K, N, K
        if fmt == GU16:
            h.chunk0 = slots
            slots += ((N + 15) // 16) * ((K + 511) // 512)
        else:
            h.chunk0, h.row0 = chunks, rows
            rows += N
            chunks += (N + 63) // 64
    p = L.EllPlanStruct()
    p.blocks_host, p.blocks_dev = C.cast(host, C.POINTER(L.EllBlock)), 0x100
    p.nblocks, p.format = len(blocks), fmt
    p.stream, p.chunk_ptr, p.chunk_len, p.perm, p.count_scratch, p.overflow = 0x200, 0x300, 0x400, 0x500, 0x600, 0x700
    p.total_rows = slots if fmt == GU16 else rows
    return p, host


def plan_string(L, c):
    """ortk_spmm_plan of the case over stand-in addresses, under the case's tuning"""
    p, host = fake_plan(L, c.fmt, [(b.N, b.K) for b in c.blocks])
    prev = L.set_tuning(**c.tuning)
    try:
        return L.spmm_plan(p, c.call, fake_args(c, L.SpmmArgs()))
    finally:
        L.set_tuning(**prev)
