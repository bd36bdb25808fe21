"""The relative-geometry attention bias (csrc/ortk_box.hip: ``ortk_box_embedding`` / ``ortk_box_logbias_fwd`` /
``ortk_box_logbias_bwd``) on a real MI355X, at every shape where one of its mechanisms becomes live (CASES below).

The reference does not recompute the embedding: two fp32 evaluations of ``sin(100 log(..) dm)`` differ by 6e-5 at arguments near
690 rad, and ``dscore / pre`` amplifies that without bound where ``pre`` is tiny.  It reads the device's own embedding ``E``
(``ortk_box_embedding``; ``pair_embedding`` is one inlined function without a contractible multiply-add, so every kernel is expected
to see the same bits) and computes everything downstream on the CPU in float64:

    pre = E . wg[l, h] + bg[l, h]            out = log(max(relu(pre), 1e-6))
    d   = dscore / pre where pre > 1e-6      dwg[l, h, :] = sum_pairs d E      dbg[l, h] = sum_pairs d

``E`` itself is compared with ``O.box_relational_embedding`` at its own bars.  Entries with -1e-4 < pre < 0.05 get dscore = 0 (at
most 3 % of a case, asserted), so that the kernel's ``pre > 1e-6`` decision cannot change a result and no large 1 / pre contributes;
nothing is excluded from a comparison.

Tolerances come from the kernels' error model, per entry and per case, never from what the kernels give:

    |d pre| <= g = 66 * 2^-24 * (sum_k |wg| |E| + |bg|)          (an fp32 dot product of 64 | 4 terms plus the bias)
    D       = 128 + ceil(nblocks / min(nblocks, 512)) + min(nblocks, 512)
              (the chain inside a block of 128 pairs, the blocks of one workgroup, at most 512 workgroup atomics)
    bound   = sum_pairs |dscore| g / (pre (pre - g)) |E| + (D + 2) 2^-24 sum_pairs |d E|      (dbg: |E| = 1)
              + min(nblocks, 512) 2^-24 |c|     where the output held c before the call (every atomic rounds at the running value)
    forward:  g / (pre - g) + 2^-23 |log pre|   (one ulp of logf)

and every comparison asserts |kernel - reference| <= 4 bound: the 4 is the margin for the compiler's reassociation inside the MFMA
chain and the rounding of the division.  Each test prints the largest error / bound it saw (profiles/box_operator_tests.txt)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import common as Cm
from oracle import ort_oracle as O

pytestmark = pytest.mark.gpu

EINVAL = -1
U = 2.0 ** -24
MARGIN = 4.0
BAND = (-1e-4, 0.05)         # ill-conditioned pre: dscore = 0 there
PAIRS, MAX_WGS = 128, 512    # ortk_box.hip: pairs per block of work, workgroups per launch
PAD = 8                      # floats of NaN on both sides of every slice
DS_PAD = 64                  # the same for dscore (a multiple of 4: the slice itself stays 16-byte aligned)

#        B,   S, H, L, trig,  dscore offset in floats
CASES = {
    "a": (3, 13, 8, 2, True, 0),       # S * S odd: scalar dscore staging; tail block with offsets of -1
    "b": (2, 36, 8, 3, True, 0),       # 16-byte staging; L = 3 reuses a score-gradient buffer and loads layer l + 2
    "c": (2, 36, 8, 3, True, 1),       # b with the dscore pointer one float further: even S on the scalar path
    "d": (5, 128, 8, 3, True, 0),      # 640 blocks > 512 workgroups: the grid-stride loop carries the workgroup's sums
    "e1": (2, 20, 4, 1, True, 0),      # H < 8: the kernel pads heads H..7 itself; L = 1
    "e2": (1, 1, 1, 1, True, 0),       # a single pair
    "f1": (3, 13, 8, 2, False, 0),     # non-trigonometric: embedding<4>, fwd<4>, bwd<4>
    "f2": (2, 36, 5, 3, False, 0),     # ... with an odd head count split over the two thread halves
    "g": (2, 36, 8, 6, True, 0),       # the model's own layer count
}
IDS = list(CASES)
SEED = {k: 100 + 10 * i for i, k in enumerate(IDS)}
SEED["c"] = SEED["b"]                  # the same inputs: c must reproduce b


@pytest.fixture(scope="module")
def L():
    import sparse_image_captioning_amd as P
    P._lib.require_gpu()
    return P._lib


def _dim_mat(trig):
    if not trig:
        return None
    dm = (1.0 / torch.pow(torch.tensor(1000.0), torch.arange(8.0) / 8.0)).numpy().astype(np.float32)
    return (C.c_float * 8)(*dm.tolist())


def _fenced(parts, pad=PAD, first=None):
    """One NaN-filled device buffer holding `parts` (fp32 CPU tensors) as slices with `pad` floats of NaN between and around them.
    Returns (buffer, [slice views], [(offset, numel)])."""
    first = pad if first is None else first
    total = first + sum(p.numel() + pad for p in parts)
    host = torch.full((total,), float("nan"))
    spans, off = [], first
    for p in parts:
        host[off:off + p.numel()] = p.reshape(-1)
        spans.append((off, p.numel()))
        off += p.numel() + pad
    buf = host.cuda()
    return buf, [buf[o:o + n] for o, n in spans], spans


def _fences_intact(buf, spans):
    keep = torch.ones(buf.numel(), dtype=torch.bool)
    for o, n in spans:
        keep[o:o + n] = False
    return bool(torch.isnan(buf.cpu()[keep]).all())


def _pp(tensors):
    return (C.c_void_p * max(len(tensors), 1))(*[t.data_ptr() for t in tensors])


_CACHE = {}


def _inputs(cid):
    """Boxes from common.make_inputs with the last regions of the last image zeroed (the executor's padded regions: w = h = 1,
    every centre difference 0), and per-layer wg = 0.3 randn, bg = 0.3 + 0.1 randn, dscore = randn: no two layers alike."""
    B, S, H, Lyr, trig, ds_off = CASES[cid]
    DG = 64 if trig else 4
    boxes = torch.from_numpy(Cm.make_inputs(SEED[cid], B, S, 4, 10, 1)["boxes"]).clone()
    if S > 1:
        boxes[-1, S - max(1, S // 4):] = 0.0
    g = torch.Generator().manual_seed(SEED[cid])
    wg = [(torch.randn(H, DG, generator=g) * 0.3).float() for _ in range(Lyr)]
    bg = [(0.3 + 0.1 * torch.randn(H, generator=g)).float() for _ in range(Lyr)]
    dscore = torch.randn(Lyr, B, H, S, S, generator=g).float()
    return dict(B=B, S=S, H=H, Lyr=Lyr, trig=trig, DG=DG, ds_off=ds_off, boxes=boxes, wg=wg, bg=bg, dscore=dscore)


def _reference(r, emb):
    """Everything downstream of the embedding `emb` (B, S, S, DG) in float64, with its bounds; zeroes dscore in the band."""
    B, S, H, Lyr, DG = r["B"], r["S"], r["H"], r["Lyr"], r["DG"]
    npairs = B * S * S
    E = emb.double().reshape(npairs, DG)
    W, Bv = torch.stack(r["wg"]).double(), torch.stack(r["bg"]).double()             # (L, H, DG), (L, H)
    pre = torch.einsum("pk,lhk->lph", E, W) + Bv[:, None, :]                         # (L, pairs, H)
    gam = 66.0 * U * (torch.einsum("pk,lhk->lph", E.abs(), W.abs()) + Bv.abs()[:, None, :])
    band = (pre > BAND[0]) & (pre < BAND[1])
    active = pre >= BAND[1]
    inactive = pre <= BAND[0]
    to_pairs = lambda t: t.reshape(Lyr, B, H, S * S).permute(0, 1, 3, 2).reshape(Lyr, npairs, H)
    from_pairs = lambda t: t.reshape(Lyr, B, S * S, H).permute(0, 1, 3, 2).reshape(Lyr, B, H, S, S)
    dscore = r["dscore"] * (~from_pairs(band)).float()                               # ill-conditioned entries carry no gradient
    ds = to_pairs(dscore.double())
    safe = torch.where(active, pre, torch.ones_like(pre))
    d = torch.where(active, ds / safe, torch.zeros_like(pre))
    amp = torch.where(active, ds.abs() * gam / (safe * (safe - gam)), torch.zeros_like(pre))
    nblocks = -(-npairs // PAIRS)
    nwg = min(nblocks, MAX_WGS)
    depth = PAIRS + -(-nblocks // nwg) + nwg
    return dict(
        r, dscore=dscore, emb=emb, nwg=nwg,
        pre=from_pairs(pre), gam=from_pairs(gam), band=from_pairs(band), active=from_pairs(active), inactive=from_pairs(inactive),
        dwg=torch.einsum("lph,pk->lhk", d, E), dbg=d.sum(1),
        dwg_bound=torch.einsum("lph,pk->lhk", amp, E.abs()) + (depth + 2) * U * torch.einsum("lph,pk->lhk", d.abs(), E.abs()),
        dbg_bound=amp.sum(1) + (depth + 2) * U * d.abs().sum(1),
        band_share=band.double().mean().item(), active_share=active.double().mean().item())


def _case(L, cid):
    """Inputs, the device's embedding and the float64 reference of one case; computed once, never modified."""
    if cid not in _CACHE:
        r = _inputs(cid)
        B, S = r["B"], r["S"]
        r["boxes_d"] = r["boxes"].cuda().contiguous()
        emb = torch.full((B, S, S, r["DG"]), float("nan"), device="cuda")
        L.check(L.lib().ortk_box_embedding(L.ptr(r["boxes_d"]), _dim_mat(r["trig"]), L.ptr(emb), B, S, L.stream_ptr()), "ortk_box_embedding")
        torch.cuda.synchronize()
        emb = emb.cpu()
        assert torch.isfinite(emb).all()
        _CACHE[cid] = _reference(r, emb)
    return _CACHE[cid]


def _forward(L, r):
    B, S, H, Lyr = r["B"], r["S"], r["H"], r["Lyr"]
    wbuf, wgd, wspans = _fenced(r["wg"])
    bbuf, bgd, bspans = _fenced(r["bg"])
    obuf, (out,), ospans = _fenced([torch.full((Lyr, B, H, S, S), float("nan"))])
    L.check(L.lib().ortk_box_logbias_fwd(L.ptr(r["boxes_d"]), _pp(wgd), _pp(bgd), _dim_mat(r["trig"]), L.ptr(out), Lyr, B, S, H,
                                         L.stream_ptr()), "ortk_box_logbias_fwd")
    torch.cuda.synchronize()
    assert _fences_intact(obuf, ospans), "the forward wrote outside its output"
    return out.cpu().reshape(Lyr, B, H, S, S)


def _pattern(n, k):
    """A non-zero fill for the gradient buffers: +-0.125 .. +-0.625."""
    i = torch.arange(n)
    return (0.125 * ((i + k) % 5 + 1).float()) * (1.0 - 2.0 * ((i + k) % 2).float())


def _backward(L, r):
    """One call into freshly allocated, fenced and pre-filled buffers.  Returns (dwg - fill, dbg - fill) in float64 plus the fills:
    the call must ADD to what the buffers hold, read nothing past a slice (NaN would reach a sum) and write nothing outside one."""
    B, S, H, Lyr, DG = r["B"], r["S"], r["H"], r["Lyr"], r["DG"]
    wbuf, wgd, wspans = _fenced(r["wg"])
    bbuf, bgd, bspans = _fenced(r["bg"])
    fill_w = [_pattern(H * DG, l) for l in range(Lyr)]
    fill_b = [_pattern(H, 3 + l) for l in range(Lyr)]
    dwbuf, dwgd, dwspans = _fenced(fill_w)
    dbbuf, dbgd, dbspans = _fenced(fill_b)
    dsbuf, (dsd,), dsspans = _fenced([r["dscore"]], pad=DS_PAD, first=DS_PAD + r["ds_off"])
    assert dsd.data_ptr() % 16 == 4 * r["ds_off"]
    w0, b0 = wbuf.clone(), bbuf.clone()
    L.check(L.lib().ortk_box_logbias_bwd(L.ptr(r["boxes_d"]), _pp(wgd), _pp(bgd), _dim_mat(r["trig"]), L.ptr(dsd), _pp(dwgd), _pp(dbgd),
                                         Lyr, B, S, H, L.stream_ptr()), "ortk_box_logbias_bwd")
    torch.cuda.synchronize()
    assert _fences_intact(dwbuf, dwspans) and _fences_intact(dbbuf, dbspans), "the backward wrote outside dwg / dbg"
    same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert same(wbuf, w0) and same(bbuf, b0), "the backward changed wg / bg"
    fw, fb = torch.stack(fill_w).reshape(Lyr, H, DG).double(), torch.stack(fill_b).double()
    dwg = torch.stack([t.cpu() for t in dwgd]).reshape(Lyr, H, DG).double()
    dbg = torch.stack([t.cpu() for t in dbgd]).double()
    assert torch.isfinite(dwg).all() and torch.isfinite(dbg).all(), "NaN reached a gradient: something was read past a slice"
    return dwg - fw, dbg - fb, fw, fb


def _bounds(r, fw, fb):
    """The reference bounds plus the rounding of the value the buffer already held, once per workgroup atomic."""
    return r["dwg_bound"] + r["nwg"] * U * fw.abs(), r["dbg_bound"] + r["nwg"] * U * fb.abs()


def _ratio(err, bound):
    """Largest error / bound; an entry whose bound is 0 (no contribution at all) must be exact."""
    zero = bound == 0
    assert (err[zero] == 0).all()
    return (err[~zero] / bound[~zero]).max().item() if (~zero).any() else 0.0


_LOG_FLOOR = []


def _log_floor(L):
    """The device's own logf(1e-6f), from a call whose every entry is inactive by construction (wg = 0, bg = -1: pre = -1 exactly).
    It is held to the forward bar at g = 0: 4 ulps of the float64 value."""
    if not _LOG_FLOOR:
        r = dict(B=1, S=3, H=2, Lyr=1, trig=True, wg=[torch.zeros(2, 64)], bg=[torch.full((2,), -1.0)],
                 boxes_d=torch.tensor([[[0.1, 0.2, 0.5, 0.6], [0.3, 0.1, 0.9, 0.4], [0.0, 0.0, 0.0, 0.0]]]).cuda())
        out = _forward(L, r).reshape(-1)
        assert (out.view(torch.int32) == out.view(torch.int32)[0]).all()
        exact = math.log(float(np.float32(1e-6)))
        assert abs(float(out[0]) - exact) <= MARGIN * 2.0 * U * abs(exact), (float(out[0]), exact)
        _LOG_FLOOR.append(out[0].clone())
    return _LOG_FLOOR[0]


@pytest.mark.parametrize("cid", IDS)
def test_inputs_are_conditioned(L, cid):
    """At most 3 % of a case's entries are ill-conditioned (and carry dscore = 0); both ReLU sides are present."""
    r = _case(L, cid)
    print(f"box {cid}: band share {r['band_share']:.4f}, active share {r['active_share']:.4f}")
    assert r["band_share"] <= 0.03
    assert (r["dscore"][r["band"]] == 0).all()
    assert r["active"].any() and (r["dscore"][r["active"]] != 0).any()
    if cid != "e2":                       # (a single entry cannot be on both sides)
        assert r["inactive"].any()
    if r["S"] > 1:
        assert (r["boxes"][-1, -1] == 0).all()


@pytest.mark.parametrize("cid", IDS)
def test_embedding_vs_oracle(L, cid):
    """The device embedding the reference is built on, against the oracle's fp32 restatement: 2e-4 for the trigonometric mode (one
    ulp of an argument near 690 rad moves sin / cos by 6e-5), the non-trigonometric golden test's 1e-4 for the log-ratios."""
    r = _case(L, cid)
    ref = O.box_relational_embedding(r["boxes"], trig=r["trig"])
    err = (r["emb"] - ref).abs().max().item()
    print(f"box {cid}: embedding max error {err:.3e}")
    if r["trig"]:
        assert err < 2e-4
    else:
        np.testing.assert_allclose(r["emb"].numpy(), ref.numpy(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("cid", IDS)
def test_forward(L, cid):
    """Inactive entries (pre <= -1e-4) are logf(1e-6f) bit for bit; well-conditioned active entries are compared as logs at
    4 (g / (pre - g) + one ulp of logf); entries in the band are finite, not below the clamp and at most log(0.05) plus that bar."""
    r = _case(L, cid)
    out = _forward(L, r)
    assert torch.isfinite(out).all()
    floor = _log_floor(L)
    ina = out[r["inactive"]]
    assert (ina.view(torch.int32) == floor.view(torch.int32)).all(), "an inactive entry is not logf(1e-6f)"
    act = r["active"]
    pre, gam = r["pre"][act], r["gam"][act]
    ref = pre.log()
    bound = gam / (pre - gam) + 2.0 * U * ref.abs()
    ratio = _ratio((out[act].double() - ref).abs(), bound)
    print(f"box {cid}: out error / bound {ratio:.4f}")
    assert ratio <= MARGIN
    band = r["band"]
    if band.any():
        hi = math.log(BAND[1]) + MARGIN * (r["gam"][band] / BAND[1] + 2.0 * U * abs(math.log(BAND[1])))
        assert (out[band].double() <= hi).all() and (out[band] >= floor).all()


@pytest.mark.parametrize("cid", IDS)
def test_backward(L, cid):
    """dwg / dbg against the float64 reference at 4 bounds, added to a non-zero fill, behind NaN fences.  A second run into fresh
    buffers agrees within 2 bounds: the kernels add their partial sums with float atomics, whose order is not fixed, so the two runs
    are NOT promised to be bit-equal."""
    r = _case(L, cid)
    dwg, dbg, fw, fb = _backward(L, r)
    wb, bb = _bounds(r, fw, fb)
    rw, rb = _ratio((dwg - r["dwg"]).abs(), wb), _ratio((dbg - r["dbg"]).abs(), bb)
    print(f"box {cid}: dwg error / bound {rw:.4f}, dbg error / bound {rb:.4f}")
    assert rw <= MARGIN and rb <= MARGIN
    dwg2, dbg2, _, _ = _backward(L, r)
    r2w, r2b = _ratio((dwg2 - dwg).abs(), wb), _ratio((dbg2 - dbg).abs(), bb)
    print(f"box {cid}: rerun dwg difference / bound {r2w:.4f}, dbg {r2b:.4f}")
    assert r2w <= 2.0 and r2b <= 2.0


def test_unaligned_dscore_matches_aligned(L):
    """Case c is case b with the dscore pointer one float past a 16-byte boundary: the scalar staging path at an even S gives what
    the 16-byte path gives, within 2 bounds."""
    rb_, rc_ = _case(L, "b"), _case(L, "c")
    assert torch.equal(rb_["dscore"], rc_["dscore"]) and torch.equal(rb_["emb"], rc_["emb"])
    dwg_b, dbg_b, fw, fb = _backward(L, rb_)
    dwg_c, dbg_c, _, _ = _backward(L, rc_)
    wb, bb = _bounds(rb_, fw, fb)
    rw, rb = _ratio((dwg_c - dwg_b).abs(), wb), _ratio((dbg_c - dbg_b).abs(), bb)
    print(f"box c vs b: dwg difference / bound {rw:.4f}, dbg {rb:.4f}")
    assert rw <= 2.0 and rb <= 2.0


def test_argument_checks(L):
    """The limits of the two entry points (include/ortk.h): H <= 8 in the backward, L <= 16, no null pointer, S >= 1, H >= 1;
    B = 0 and L = 0 are valid, empty calls that write nothing."""
    lib, st = L.lib(), L.stream_ptr()
    B, S, H, Lyr = 2, 5, 4, 2
    dm = _dim_mat(True)
    boxes = torch.rand(B, S, 4).cuda()
    big = [torch.zeros(9 * 64).cuda() for _ in range(17)]
    small = [torch.zeros(9).cuda() for _ in range(17)]
    mark = lambda: [torch.full((9 * 64,), 7.0).cuda() for _ in range(17)]
    dw, db = mark(), mark()
    ds = torch.ones(17 * B * 9 * S * S).cuda()
    out = torch.full((17 * B * 9 * S * S,), 7.0).cuda()
    bwd = lambda L_, B_, S_, H_, dsp=L.ptr(ds): lib.ortk_box_logbias_bwd(L.ptr(boxes), _pp(big), _pp(small), dm, dsp, _pp(dw), _pp(db),
                                                                          L_, B_, S_, H_, st)
    fwd = lambda L_, B_, S_, H_: lib.ortk_box_logbias_fwd(L.ptr(boxes), _pp(big), _pp(small), dm, L.ptr(out), L_, B_, S_, H_, st)
    assert bwd(Lyr, B, S, 9) == EINVAL
    assert bwd(17, B, S, H) == EINVAL
    assert bwd(Lyr, B, S, H, None) == EINVAL
    assert bwd(Lyr, B, 0, H) == EINVAL
    assert fwd(17, B, S, H) == EINVAL
    assert fwd(Lyr, B, S, 0) == EINVAL
    assert bwd(Lyr, 0, S, H) == 0 and bwd(0, B, S, H) == 0
    assert fwd(Lyr, 0, S, H) == 0 and fwd(0, B, S, H) == 0
    torch.cuda.synchronize()
    assert all((t == 7.0).all() for t in dw + db) and (out == 7.0).all()
