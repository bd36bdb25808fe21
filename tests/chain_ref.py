"""Float64 reference, fp32 error model, launch geometry and exact "routing" operands of the rows-stationary chains (csrc/ortk_chain.hip:
row_chain_kernel, row_chain_wide_kernel, row_bchain_kernel).  numpy only, no GPU.  tests/test_chain_ref_host.py shows on the CPU that the
bars below are sound (an fp32 restatement of every stage stays within 1 bound) and sharp (eight mutants are caught);
tests/test_gpu_row_chain.py holds the kernels to them.

The operators (include/ortk.h: ortk_chain_args / ortk_bchain_args; the reference's models/transformer.py:293-294 SublayerConnection,
324-325 PositionwiseFeedForward, 338-341 LayerNorm), per row, d = 512, d_ff = 512 NC, keep = the dropout draw of the element times
1 / (1 - p):

    R    x_mid = x_in + keep_r (a_in Wr^T + bias_r)
    L1   y1, st1 = LayerNorm(x_mid; g1, b1)                          (ln_ref.forward: unbiased std, eps outside the root)
    S1   out1[:, 512 i ..] = y1 W_i^T + bias_s1[512 i ..]
    F    h = keep_h relu(y1 W1^T + bias_h)          x_out = x_mid + keep_o (h W2^T + bias_o)
    L2   y2, st2 = LayerNorm(x_out; g2, b2)         S2   out2 as S1 from y2

    P0   gy = sum_i ain[:, 512 i ..] U_i            LNa  dxa = LayerNorm'(gy; xa, sta, ga) + dresa    (ln_ref.backward), daa / dba += sums
         dza = keep_a dxa (bf16)                    P1   gh = [hgate > 0] gate_scale (dz W2)  (bf16),   gy2 = gh W1
    LNb  dxb = LayerNorm'(gy2; xb, stb, gb) + dresb,  dzb = keep_b dxb                P2   out2 = dz Wo  (bf16)

EVERY STAGE IS COMPUTED FROM THE KERNEL'S OWN STORED INPUT OF THAT STAGE (forward_stages / backward_stages take the stored tensors):
x_mid from x_in and a_in; the statistics and y1 from the stored x_mid; out1 and h from the stored (bf16) y1; x_out from the stored x_mid
and h; y2 / st2 from the stored x_out; out2 from the stored y2 -- dxa from ain; dza from the stored dxa; gh from the stored dza (or
dz0); dxb from the stored gh (and the stored dxa as dresb); dzb from the stored dxb; out2 from the stored dzb / dza / dz0.  No stage's
rounding hides the next one's, and every bound below is the bound of ONE stage.

Error model.  u = 2^-24, worst case, linear in the number of terms, per entry:

    product   a product of two bf16 values is exact in fp32, so a K-term unit (any summation order, the matrix cores' included) is
              within (K + 2) u sum|a||w| of the exact sum; K = 512, or d_ff for the FFN's second product (ONE running sum over the
              chunks, ortk_chain.hip:356 / 659), or 512 nin for P0 (ortk_chain.hip:836-837)
    + u |v|   for each of: the bias add, the dropout scale (keep is the kernel's own fp32 1 / (1 - p), an input of the reference),
              the residual add, the gate scale
    LayerNorm ln_ref.forward_bound / backward_bound with D = D_CHAIN = 22: a lane's chain of 16 values (4 column tiles x 4 registers,
              ortk_chain.hip:222-226 / 536-540; the backward 778-782), two shuffles (227 / 541 / 783-784), three levels over the eight
              column waves' LDS partials (233-234 / 547-548 / 790-793; the second exchange 246-247 / 560-561 is the same tree), the
              scaling by 1 / n: 16 + 2 + 3 + 1.  The backward is handed statistics that are the fp32 rounding of the float64 ones:
              inside d_mean / d_sd.  Its dy is a product: e = (K + 2) u sum|a||w| enters as ln_ref's `e`.
    da / db   a block adds its rows' terms: a chain over its 3 row tiles, four shuffle levels over the 16 rows of a tile
              (ortk_chain.hip:745-771), ONE float atomic per block and column: ln_ref.colsum_bound(levels = 7, nblocks = workgroups)

fp32 outputs (x_mid, x_out, st1, st2, dxa, dxb, da, db) assert |kernel - reference| <= MARGIN x bound, MARGIN = ln_ref.MARGIN = 4.
bf16 outputs (y1, y2, out1, out2, h, dza, dzb, gh) are checked as an INTERVAL: the stored value lies between bf16_rn(ref - 4 bound) and
bf16_rn(ref + 4 bound) -- the kernel rounds an fp32 value inside [ref - 4 bound, ref + 4 bound] once, and rounding is monotone.  That
admits a second bf16 value only where the true value sits within 4 bounds of a rounding boundary.  interval_miss returns the entries
outside and how far outside, in units of the bound.  No constant is taken from what a kernel returns.

Routing operands (routing_unit, routing_stack, routing_w2): every 512 x 512 unit is a signed selection matrix -- output j takes c_j x input pi(j),
c_j in {+-1, +-2, +-1/2}, pi a seeded permutation that differs per unit -- so a product is ONE exact term: out1[:, 512 i + j] ==
c y1[:, pi_i(j)] (zero projection bias), h == bf16_rn(keep relu(c y1[:, pi(j)] + bias_h[j])), x_out == x_mid + keep (c h[:, sigma(j)] +
bias_o[j]) with the roundings of single fp32 operations (numpy float32), exactly, and with p = 0.5 the scale is exactly 2.  W2 selects
every hidden unit at most once over ALL chunks: output j reads hidden unit sigma(j) of chunk sigma(j) // 512 and nothing of the other
chunks.  A wrong unit offset or leading dimension, swapped W1 / W2 chunks, a lost k-step or a wrong column tile is a value mismatch at
a known (row, column).

Geometry (rows_per_block, is_wide, plan): a restatement of the launcher (ortk_chain.hip: chain_rows_per_block, chain_wide, chain_geom),
asserted equal to ortk_row_chain_plan / ortk_row_bchain_plan by the host test.

Dropout draws (keep): a restatement of csrc/ortk_common.h: ortk_keep4_u32, element index = key row x row length + column."""
import numpy as np

import ln_ref as R

U, MARGIN = R.U, R.MARGIN
D_MODEL = 512
D_CHAIN = 22
COLSUM_LEVELS = 7                # 3 row tiles in a chain + four shuffle levels
NARROW_ROWS, WIDE_ROWS, SLOTS = 48, 76, 256


# ------------------------------------------------------------------------------------------------ geometry
def _cdiv(a, b):
    return -(-a // b)


def rows_per_block(M, slots=SLOTS):
    """Rows a workgroup of the 48-row kernels owns: the fewest rounds of `slots` workgroups, the rows spread evenly over them."""
    rounds = _cdiv(_cdiv(M, NARROW_ROWS), slots)
    return min(NARROW_ROWS, max(_cdiv(M, rounds * slots), 1))


def is_wide(M, chain_wide=1, progress=False):
    """The 76-row form: never with prefetchers; chain_wide 1 where ONE round of it replaces two narrow ones, 2 wherever it saves one."""
    if progress or not chain_wide:
        return False
    rw, rn = _cdiv(_cdiv(M, WIDE_ROWS), SLOTS), _cdiv(_cdiv(M, NARROW_ROWS), SLOTS)
    return rw < rn if chain_wide == 2 else (rw == 1 and rn == 2)


def plan(M, chain_wide=1, progress=False):
    """What ortk_row_chain_plan returns, + `last` (rows of the last block) and `rounds`."""
    wide, npf = is_wide(M, chain_wide, progress), 8 if progress else 0
    slots = SLOTS - npf
    rb = min(WIDE_ROWS, _cdiv(M, _cdiv(_cdiv(M, WIDE_ROWS), SLOTS) * SLOTS)) if wide else rows_per_block(M, slots)
    wg = _cdiv(M, rb)
    return dict(form=int(wide), rows_per_block=rb, workgroups=wg, prefetchers=npf, last=M - (wg - 1) * rb, rounds=_cdiv(wg, slots))


def bplan(M):
    rb = rows_per_block(M)
    wg = _cdiv(M, rb)
    return dict(rows_per_block=rb, workgroups=wg, last=M - (wg - 1) * rb)


def geometry_classes(M, chain_wide=1, progress=False):
    """Names of the geometry classes a forward case of M rows hits (the host test asserts the case table covers ALL_CLASSES)."""
    g = plan(M, chain_wide, progress)
    rb, last, out = g["rows_per_block"], g["last"], set()
    out.add(("wide" if g["form"] else "narrow") + f":rb={rb}")
    if not g["form"]:
        if rb == 1: out.add("narrow:one-row blocks, tiles 1 and 2 empty")
        if rb == 16 and last == 16: out.add("narrow:tile boundary 16, full")
        if rb == 16 and last < 16: out.add("narrow:tile boundary 16, partial last block")
        if rb == 17: out.add("narrow:tile boundary 17")
        if rb == 32: out.add("narrow:tile boundary 32")
        if rb == 33: out.add("narrow:tile boundary 33")
        if rb == 48 and last == 48: out.add("narrow:48 rows, full")
        if rb == 48 and last < 48: out.add("narrow:48 rows, partial last block")
        if g["rounds"] == 2: out.add("narrow:two rounds" + (" with prefetchers" if progress else ""))
        if progress and g["rounds"] == 1: out.add("narrow:one round with prefetchers")
    else:
        if rb == 49: out.add("wide:49 rows")
        if rb == 64: out.add("wide:64 rows, fifth tile empty")
        if rb == 65: out.add("wide:65 rows")
        if rb == 76 and last == 76: out.add("wide:76 rows, full")
        if rb == 76 and last < 76: out.add("wide:76 rows, partial last block")
        if g["rounds"] == 2: out.add("wide:two rounds")
    return out


ALL_CLASSES = {"narrow:one-row blocks, tiles 1 and 2 empty", "narrow:tile boundary 16, full", "narrow:tile boundary 16, partial last block",
               "narrow:tile boundary 17", "narrow:tile boundary 32", "narrow:tile boundary 33", "narrow:48 rows, full",
               "narrow:48 rows, partial last block", "narrow:two rounds", "narrow:one round with prefetchers", "narrow:two rounds with prefetchers",
               "wide:49 rows", "wide:64 rows, fifth tile empty", "wide:65 rows", "wide:76 rows, full", "wide:76 rows, partial last block",
               "wide:two rounds"}

# The case table of tests/test_gpu_row_chain.py: (M, chain_wide, progress) -> (form, rb, workgroups, rows of the last block), the
# values of the issue's tables, computed on the CPU from the launcher's formula and asserted by the host test against this restatement
# AND the plan query.
GEOMETRY_CASES = {
    (1, 1, 0): (0, 1, 1, 1), (256, 1, 0): (0, 1, 256, 1), (257, 1, 0): (0, 2, 129, 1), (4090, 1, 0): (0, 16, 256, 10),
    (4096, 1, 0): (0, 16, 256, 16), (4100, 1, 0): (0, 17, 242, 3), (8192, 1, 0): (0, 32, 256, 32), (8200, 1, 0): (0, 33, 249, 16),
    (12000, 1, 0): (0, 47, 256, 15), (12280, 1, 0): (0, 48, 256, 40), (12288, 1, 0): (0, 48, 256, 48),
    (12289, 0, 0): (0, 25, 492, 14),
    (1, 1, 1): (0, 1, 1, 1), (11904, 1, 1): (0, 48, 248, 48), (11905, 1, 1): (0, 25, 477, 5),
    (12289, 1, 0): (1, 49, 251, 39), (16384, 1, 0): (1, 64, 256, 64), (16385, 1, 0): (1, 65, 253, 5), (19450, 1, 0): (1, 76, 256, 70),
    (19456, 1, 0): (1, 76, 256, 76), (19457, 1, 0): (0, 39, 499, 35),
    (24577, 2, 0): (1, 49, 502, 28),
}
BWD_ROWS = (1, 257, 4100, 8200, 12288)


# ------------------------------------------------------------------------------------------------ number formats, dropout draws
def bf16_rn(x):
    """Round-to-nearest-even to bf16 of the fp32 rounding of x, as float32 (finite values)."""
    b = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)
    return ((b + (((b >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)).view(np.float32)


def _mix32(x):
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def keep(seed, keys, ncols, p, row_len=None):
    """(rows, ncols) bool: element (key row, column) of a (., row_len) tensor is kept (ortk_common.h: ortk_keep4_u32 / ortk_keep_u32)."""
    row_len = ncols if row_len is None else row_len
    with np.errstate(over="ignore"):
        idx = np.asarray(keys, dtype=np.uint32)[:, None] * np.uint32(row_len) + np.arange(ncols, dtype=np.uint32)[None, :]
        h = _mix32((idx >> np.uint32(2)) * np.uint32(0x9E3779B1) + np.uint32(seed))
        g = (h ^ np.uint32(0x68E31DA4)) * np.uint32(0xB5297A4D)
        g = g ^ (g >> np.uint32(15))
    w = np.where(idx & np.uint32(2), g, h)
    f = (w >> ((idx & np.uint32(1)) * np.uint32(16))) & np.uint32(0xFFFF)
    return f >= np.uint32(int(np.float32(p) * np.float32(65536.0)))


def keep_scale(p):
    """The kernels' fp32 1 / (1 - p)."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p)) if p > 0 else np.float32(1.0)


# ------------------------------------------------------------------------------------------------ bounds and checks
# Two arithmetics for the products and the bf16 comparisons, the big tensors of a case: numpy float64 (device = None), or torch float64
# on `device` for the tall cases (the products alone are about 0.1 TFLOP there); one GPU case computes both and asserts they agree.
# The LayerNorm parts and every fp32 output are numpy float64 always (ln_ref).
def _f64(t):
    """numpy float64 of a numpy array, a scalar or a torch tensor."""
    if hasattr(t, "detach"):
        return t.detach().double().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def _on(t, device):
    """t as float64 in the arithmetic of `device` (None: numpy)."""
    if device is None:
        return _f64(t)
    import torch
    if isinstance(t, torch.Tensor):
        return t.to(device=device, dtype=torch.float64)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.float64))).to(device)


def _like(t, ref):
    return _on(t, None if isinstance(ref, np.ndarray) else ref.device)


def _bf16_rn64(x):
    """bf16_rn in the arithmetic of x, as float64."""
    if isinstance(x, np.ndarray):
        return bf16_rn(x).astype(np.float64)
    return x.float().bfloat16().double()


def _finite(x):
    return bool((abs(x) < float("inf")).all())


def product(a, w, bias=None, device=None):
    """a w^T (+ bias) in float64 and the bound of its fp32 evaluation: (K + 2) u sum|a||w| (+ u |v| for the bias add)."""
    a, w = _on(a, device), _on(w, device)
    v = a @ w.T
    b = (a.shape[1] + 2) * U * (abs(a) @ abs(w).T)
    if bias is not None:
        v = v + _on(bias, device)
        b = b + U * abs(v)
    return v, b


def interval_miss(stored, ref, bound, lo_clip=None):
    """bf16 interval check: the largest distance of a stored value outside [bf16_rn(ref - 4 bound), bf16_rn(ref + 4 bound)], in units
    of the bound (0.0: all inside), and the number of entries outside."""
    if isinstance(ref, np.ndarray):
        bound = np.broadcast_to(_f64(bound), ref.shape)
    stored, bound = _like(stored, ref), _like(bound, ref)
    assert _finite(stored) and _finite(ref)
    lo, hi = ref - MARGIN * bound, ref + MARGIN * bound
    if lo_clip is not None:
        lo, hi = lo.clip(min=lo_clip), hi.clip(min=lo_clip)
    lo, hi = _bf16_rn64(lo), _bf16_rn64(hi)
    out = (stored < lo) | (stored > hi)
    if not bool(out.any()):
        return 0.0, 0
    dist = ((lo - stored).clip(min=0) + (stored - hi).clip(min=0))[out]
    bo = bound[out]
    return (float((dist / bo).max()) if bool((bo > 0).all()) else float("inf")), int(out.sum())


def bf16_interval_ratio(stored, ref, bound):
    """How far inside the model the bf16 values sit: the largest |stored - ref| minus half a bf16 step of the stored value, over the
    bound (printed, not asserted: the interval is the assertion)."""
    if isinstance(ref, np.ndarray):
        bound = np.broadcast_to(_f64(bound), ref.shape)
    stored, bound = _like(stored, ref), _like(bound, ref)
    step = abs(stored) * 2.0 ** -8 + 2.0 ** -134
    ex = (abs(stored - ref) - step).clip(min=0)
    nz = bound > 0
    return float((ex[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


def forward_stages(t, w, p=0.0, eps=R.EPS, device=None):
    """Reference and bound of every stage of a forward chain.  t: the tensors (x_in, a_in, and the kernel's STORED x_mid, y1, h, x_out,
    y2 as far as the chain has them; numpy or torch), w: the operands (Wr, bias_r, g1, b1, S1 (n1 512, 512), bias_s1, W1, bias_h, W2,
    bias_o, g2, b2, S2, bias_s2) and the keep factors keep_r / keep_h / keep_o (0 or the kernel's 1 / (1 - p); absent = 1).  Returns
    {name: (ref, bound)} for the outputs the chain has; st1 / st2 as (rows, 2) of {mean, std}.  device: see above; out1, h, out2 stay in
    that arithmetic, everything else is numpy."""
    out = {}
    x1 = t["x_in"]
    if "Wr" in w:
        v, b = (_f64(z) for z in product(t["a_in"], w["Wr"], w["bias_r"], device))
        k = _f64(w.get("keep_r", 1.0))
        ref = _f64(t["x_in"]) + k * v
        out["x_mid"] = (ref, k * b + (U * np.abs(k * v) if p > 0 else 0.0) + U * np.abs(ref))
        x1 = t["x_mid"]

    def ln(x, g, bb, ny, ns):
        y, mean, sd = R.forward(_f64(x), g, bb, eps)
        by, bm, bs = R.forward_bound(_f64(x), g, bb, eps, D=D_CHAIN)
        out[ny] = (y, by)
        out[ns] = (np.stack([mean, sd], 1), np.stack([bm, bs], 1))

    if "g1" in w:
        ln(x1, w["g1"], w["b1"], "y1", "st1")
        if "S1" in w:
            out["out1"] = product(t["y1"], w["S1"], w["bias_s1"], device)
    x2 = x1
    if "W1" in w:
        v, b = product(t["y1"], w["W1"], w["bias_h"], device)
        k = _on(w.get("keep_h", 1.0), device)
        ref = k * v.clip(min=0)
        out["h"] = (ref, k * b + (U * abs(ref) if p > 0 else 0.0))
        v, b = (_f64(z) for z in product(t["h"], w["W2"], w["bias_o"], device))
        k = _f64(w.get("keep_o", 1.0))
        ref = _f64(x1) + k * v
        out["x_out"] = (ref, k * b + (U * np.abs(k * v) if p > 0 else 0.0) + U * np.abs(ref))
        x2 = t["x_out"]
    if "g2" in w:
        ln(x2, w["g2"], w["b2"], "y2", "st2")
        if "S2" in w:
            out["out2"] = product(t["y2"], w["S2"], w["bias_s2"], device)
    return out


def backward_stages(t, w, workgroups, eps=R.EPS, p=0.0, device=None):
    """As forward_stages for ortk_row_bchain.  t: ain | dz0, xa, xb, dresa, hgate and the STORED dxa, dza, gh, dxb, dzb; dresb (what the
    LNb residual gradient is: the stored dxa where it is aliased); ca / cb: what daa, dba / dab, dbb held before ((2, 512) each).
    w: Win (512 nin, 512): gy = ain Win; W2 (512, d_ff), W1 (d_ff, 512), Wo (512, 512); ga, gb; keep_a / keep_b; gate_scale.
    gh stays in the arithmetic of `device`."""
    out = {}
    dz = t.get("dz0")
    opt = lambda k: None if t.get(k) is None else _f64(t[k])
    if "Win" in w:
        gy, e = (_f64(z) for z in product(t["ain"], _f64(w["Win"]).T, None, device))
        dx, da, db = R.backward(gy, _f64(t["xa"]), w["ga"], eps, dres=opt("dresa"))
        bdx, ea, ta, eb, tb = R.backward_bound(gy, _f64(t["xa"]), w["ga"], eps, dres=opt("dresa"), D=D_CHAIN, e=e)
        ca = _f64(t["ca"])
        out["dxa"] = (dx, bdx)
        out["daa"] = (da + ca[0], R.colsum_bound(ea, ta, COLSUM_LEVELS, workgroups, ca[0]))
        out["dba"] = (db + ca[1], R.colsum_bound(eb, tb, COLSUM_LEVELS, workgroups, ca[1]))
        out["_rerun_a"] = (ta, tb)
        if "keep_a" in w:
            ref = _f64(w["keep_a"]) * _f64(t["dxa"])
            out["dza"] = (ref, U * np.abs(ref) if p > 0 else np.zeros_like(ref))
            dz = t["dza"]
    if "W2" in w:
        v, b = product(dz, _f64(w["W2"]).T, None, device)
        gate = (_on(t["hgate"], device) > 0) * float(w["gate_scale"])
        ref = gate * v
        out["gh"] = (ref, gate * b + (U * abs(ref) if w["gate_scale"] != 1.0 else 0.0))
        gy, e = (_f64(z) for z in product(t["gh"], _f64(w["W1"]).T, None, device))
        dx, da, db = R.backward(gy, _f64(t["xb"]), w["gb"], eps, dres=opt("dresb"))
        bdx, ea, ta, eb, tb = R.backward_bound(gy, _f64(t["xb"]), w["gb"], eps, dres=opt("dresb"), D=D_CHAIN, e=e)
        cb = _f64(t["cb"])
        out["dxb"] = (dx, bdx)
        out["dab"] = (da + cb[0], R.colsum_bound(ea, ta, COLSUM_LEVELS, workgroups, cb[0]))
        out["dbb"] = (db + cb[1], R.colsum_bound(eb, tb, COLSUM_LEVELS, workgroups, cb[1]))
        out["_rerun_b"] = (ta, tb)
        if "keep_b" in w:
            ref = _f64(w["keep_b"]) * _f64(t["dxb"])
            out["dzb"] = (ref, U * np.abs(ref) if p > 0 else np.zeros_like(ref))
            dz = t["dzb"]
    if "Wo" in w:
        out["out2"] = tuple(_f64(z) for z in product(dz, _f64(w["Wo"]).T, None, device))
    return out


FP32_OUTPUTS = ("x_mid", "x_out", "st1", "st2", "dxa", "dxb", "daa", "dba", "dab", "dbb")


def measure(stored, stages):
    """{name: (largest error / bound, entries outside the bar)} of every stage present in `stored`: fp32 outputs against MARGIN x
    bound, bf16 outputs against the interval (their ratio is bf16_interval_ratio)."""
    res = {}
    for name, (ref, bound) in stages.items():
        if name.startswith("_") or name not in stored or stored[name] is None:
            continue
        got = _like(stored[name], ref)
        if not _finite(got):
            res[name] = (float("inf"), int((~(abs(got) < float("inf"))).sum()))
        elif name in FP32_OUTPUTS:
            bound = np.broadcast_to(_f64(bound), ref.shape)
            err = np.abs(got - ref)
            res[name] = (R.ratio(err, bound), int((err > MARGIN * bound).sum()))
        else:
            _, n = interval_miss(got, ref, bound, lo_clip=0.0 if name == "h" else None)
            res[name] = (bf16_interval_ratio(got, ref, bound), n)
    return res


def check(stored, stages, tag="", verbose=True):
    """Assert every stage present in `stored`: finite, fp32 outputs |error| <= MARGIN bound, bf16 outputs inside their interval.
    Returns {name: largest error / bound}; prints it."""
    res = measure(stored, stages)
    if verbose:
        print(f"chain {tag}: error / bound " + ", ".join(f"{k} {v[0]:.4f}" for k, v in res.items()))
    for name, (ratio, n) in res.items():
        assert np.isfinite(ratio), f"{tag} {name}: {n} entries not finite"
        assert n == 0, f"{tag} {name}: {n} entries outside the bar, error / bound {ratio:.3f}"
    return {k: v[0] for k, v in res.items()}


# ------------------------------------------------------------------------------------------------ routing operands
COEFS = np.array([1.0, -1.0, 2.0, -2.0, 0.5, -0.5])


def routing_unit(seed):
    """(W (512, 512) float32, pi, c): W[j, pi[j]] = c[j], one non-zero per output row, pi a permutation."""
    g = np.random.default_rng(seed)
    pi, c = g.permutation(D_MODEL), COEFS[g.integers(0, len(COEFS), D_MODEL)]
    W = np.zeros((D_MODEL, D_MODEL), dtype=np.float32)
    W[np.arange(D_MODEL), pi] = c
    return W, pi, c


def routing_stack(n, seed):
    """n units stacked as the rows of one (512 n, 512) matrix (S1 / S2 / W1): (W, pi (n, 512), c (n, 512))."""
    us = [routing_unit(seed + 7919 * i) for i in range(n)]
    return np.concatenate([u[0] for u in us]), np.stack([u[1] for u in us]), np.stack([u[2] for u in us])


def routing_w2(NC, seed):
    """(W2 (512, 512 NC), sigma, c): output j reads hidden unit sigma[j] (one of ALL 512 NC, every unit at most once) x c[j]."""
    g = np.random.default_rng(seed)
    sigma, c = g.permutation(D_MODEL * NC)[:D_MODEL], COEFS[g.integers(0, len(COEFS), D_MODEL)]
    W = np.zeros((D_MODEL, D_MODEL * NC), dtype=np.float32)
    W[np.arange(D_MODEL), sigma] = c
    return W, sigma, c


def route(x, pi, c):
    """x W^T of a routing unit, exactly (float32): out[:, j] = c[j] x[:, pi[j]]."""
    return (np.asarray(x, dtype=np.float32)[:, pi] * c.astype(np.float32)[None, :]).astype(np.float32)


def route_stack(x, pi, c):
    return np.concatenate([route(x, pi[i], c[i]) for i in range(pi.shape[0])], axis=1)


def routing_forward(t, r, keeps):
    """The exact values of a full routing chain from the kernel's stored stage inputs: x_mid, out1, h, x_out, out2 (float32; the bf16
    ones as their float32 values).  r: Wr = (pi, c), bias_r, S1 = (pi, c), W1 = (pi, c), bias_h, W2 = (sigma, c), bias_o, S2 = (pi, c);
    keeps: keep_r / keep_h / keep_o as float32 factors (0 or 1 / (1 - p))."""
    f32 = np.float32
    out = {}
    v = (route(t["a_in"], *r["Wr"]) + r["bias_r"].astype(f32)[None, :]).astype(f32)
    out["x_mid"] = (t["x_in"].astype(f32) + (v * keeps["keep_r"].astype(f32)).astype(f32)).astype(f32)
    out["out1"] = route_stack(t["y1"], *r["S1"])
    v = np.maximum((route_stack(t["y1"], *r["W1"]) + r["bias_h"].astype(f32)[None, :]).astype(f32), f32(0))
    out["h"] = bf16_rn((v * keeps["keep_h"].astype(f32)).astype(f32))
    sigma, c = r["W2"]
    v = (route(t["h"], sigma, c) + r["bias_o"].astype(f32)[None, :]).astype(f32)
    out["x_out"] = (t["x_mid"].astype(f32) + (v * keeps["keep_o"].astype(f32)).astype(f32)).astype(f32)
    out["out2"] = route_stack(t["y2"], *r["S2"])
    return out
