"""The partials form of the width-512 LayerNorm backward on a real MI355X: ortk_layernorm_bwd_part leaves one [2][512] block of column
sums per workgroup and issues no atomic, ortk_ln_partials_reduce adds any number of such slots into their da / db in one launch.

Against the atomics form (ortk_layernorm_bwd_dt; in the executor ortk_tuning.ln_fuse = 16): dx and dz bit-identical.  Against the
float64 reference of tests/ln_ref.py: da / db within MARGIN = 4 bounds of its error model, with the summation shape of this form:

    a wave's chain of ceil(rpb / 4) rows, two levels over the four waves            (the block, as in the atomics form)
    a thread's chain of ceil(ceil(nblocks / 32) / 4) blocks, two levels over its four accumulators, five levels over the 32 block lanes
    ONE atomic per column at the running value c                                      (colsum_bound with nblocks = 1)

where rpb = the rows a workgroup walks: ortk_ln_part_rows() = 16, more where the cap of 512 blocks asks for it.  Inputs, fences and the
reference are those of tests/test_gpu_layernorm.py (row i of class i mod 5 of ln_ref.class_rows; every buffer between NaN fences)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ln_ref as R
import test_gpu_layernorm as T

pytestmark = pytest.mark.gpu

EINVAL = -1
EPS, U, MARGIN = R.EPS, R.U, R.MARGIN
RPB, CAP = 16, 512
SPARE = 3                 # blocks of NaN behind the ones a launch may write


@pytest.fixture(scope="module")
def L():
    import sparse_image_captioning_amd as P
    P._lib.require_gpu()
    assert P._lib.lib().ortk_ln_part_rows() == RPB
    return P._lib


def _shape(rows):
    """(rows a workgroup walks, blocks) of a launch over `rows` rows."""
    rpb = max(RPB, -(-rows // CAP))
    return rpb, -(-rows // rpb)


def _levels(rows):
    rpb, nb = _shape(rows)
    return -(-rpb // 4) + 2 + -(-(-(-nb // 32)) // 4) + 2 + 5


#          dres    dz: None | (p, keyed)
OPTIONS = [(wr, dz) for wr in (False, True) for dz in (None, (0.1, False), (0.1, True))]


def _run(L, c, form, with_res, dz, prior=True):
    """One backward of case `c` into fresh fenced buffers.  form "atomics": ortk_layernorm_bwd_dt.  form "partials":
    ortk_layernorm_bwd_part into a NaN-filled partials buffer + ONE ortk_ln_partials_reduce.  Returns dx, da, db, dz (and the blocks of partials) on the CPU."""
    rows, d = c["rows"], c["d"]
    lib, bf = L.lib(), c["dy"].dtype == torch.bfloat16
    fx, fdy = T.Fenced([T._t(c["x"])]), T.Fenced([c["dy"]], c["dy"].dtype)
    fin = T.Fenced([T._t(c["a"]), c["st"], T._t(c["dres"])])
    fdx = T.Fenced([T._nan(rows * d)])
    fg = T.Fenced([T._t(c["ca"]), T._t(c["cb"])] if prior else [torch.zeros(d), torch.zeros(d)])
    fdz = T.Fenced([T._nan(rows * d)], torch.bfloat16)
    p, keyed = dz if dz else (0.0, False)
    rows_d = T._t(c["perm"]).cuda() if keyed else None
    common = (L.ptr(fdz.views[0]) if dz else None, 1, p, T.DROP_SEED, L.ptr(rows_d), L.stream_ptr())
    ins = (L.ptr(fdy.views[0]), int(bf), L.ptr(fx.views[0]), L.ptr(fin.views[0]), L.ptr(fin.views[1]), L.ptr(fin.views[2]) if with_res else None,
           L.ptr(fdx.views[0]))
    fences, blocks = [fx, fdy, fin, fdx, fg, fdz], None
    if form == "atomics":
        L.check(lib.ortk_layernorm_bwd_dt(*ins, L.ptr(fg.views[0]), L.ptr(fg.views[1]), rows, d, EPS, *common), "ortk_layernorm_bwd_dt")
    else:
        want = _shape(rows)[1]
        fpart = T.Fenced([T._nan((want + SPARE) * 2 * d)])
        fences.append(fpart)
        nb = C.c_int32(-1)
        L.check(lib.ortk_layernorm_bwd_part(*ins, L.ptr(fpart.views[0]), want, C.byref(nb), rows, d, EPS, *common), "ortk_layernorm_bwd_part")
        torch.cuda.synchronize()
        assert nb.value == want == lib.ortk_ln_part_blocks(rows)
        part = fpart.views[0].reshape(want + SPARE, 2 * d)
        assert torch.isfinite(part[:want]).all() and torch.isnan(part[want:]).all(), "a block not written, or one written behind nblocks"
        slot = L.LnSlot(fpart.views[0].data_ptr(), want, fg.views[0].data_ptr(), fg.views[1].data_ptr())
        L.check(lib.ortk_ln_partials_reduce(C.byref(slot), 1, L.stream_ptr()), "ortk_ln_partials_reduce")
        torch.cuda.synchronize()
        assert torch.isnan(part[want:]).all()
        blocks = part[:want].cpu()
    torch.cuda.synchronize()
    assert all(f.intact() for f in fences), "a write outside an output"
    dx, dzo = fdx.views[0].cpu().reshape(rows, d), fdz.views[0].cpu().reshape(rows, d)
    da, db = fg.views[0].cpu(), fg.views[1].cpu()
    assert torch.isfinite(dx).all() and torch.isfinite(da).all() and torch.isfinite(db).all(), "a NaN: an entry not written, or a read behind nblocks"
    if not dz:
        assert torch.isnan(dzo.float()).all(), "dz = NULL, and something was written"
        dzo = None
    return dx, da, db, dzo, blocks


@pytest.mark.parametrize("bf16_dy", [False, True], ids=["f32dy", "bf16dy"])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, RPB - 1, RPB, RPB + 1, 2 * RPB + 3, CAP * RPB + 3])
def test_partials_and_reduce_against_the_atomics_form_and_the_reference(L, rows, bf16_dy):
    """Every option set (dres NULL / given; dz NULL / bf16 with dropout 0.1 / the same keyed by drop_rows) at every row count around a
    wave round and a block, and at 8 195 rows, where the cap makes a workgroup walk 17 rows: dx / dz bit-equal to the atomics form, da / db
    within 4 bounds of the float64 reference on top of their prior content, bit-equal on a rerun, blocks behind nblocks untouched."""
    c = T._bwd_case(L, rows, 512, bf16_dy)
    lv = _levels(rows)
    ea, ta, eb, tb = R.backward_bound(c["dy"].float().numpy(), c["x"], c["a"])[1:]
    ba, bb = R.colsum_bound(ea, ta, lv, 1, c["ca"]), R.colsum_bound(eb, tb, lv, 1, c["cb"])
    for with_res, dz in OPTIONS:
        ref = _run(L, c, "atomics", with_res, dz)
        out = _run(L, c, "partials", with_res, dz)
        assert T._same(out[0], ref[0]), "dx differs from the atomics form"
        assert dz is None or T._same(out[3], ref[3]), "dz differs from the atomics form"
        r = (R.ratio(np.abs(T._np64(out[1]) - (c["ca"] + c["da"])), ba), R.ratio(np.abs(T._np64(out[2]) - (c["cb"] + c["db"])), bb))
        print(f"ln partials rows={rows} {'bf16' if bf16_dy else 'f32'} dy, dres {with_res}, dz {dz}: da error / bound {r[0]:.4f}, db {r[1]:.4f}")
        assert max(r) <= MARGIN
        again = _run(L, c, "partials", with_res, dz)
        assert T._same(again[1], out[1]) and T._same(again[2], out[2]), "a rerun changed bits of da / db"


def test_slots_of_different_block_counts_and_a_shared_destination(L):
    """Three slots in ONE reduce call: 3 blocks and 1 block into one destination (shared layers), the 1 block again into another."""
    lib = L.lib()
    cA, cB = T._bwd_case(L, 2 * RPB + 3, 512, True), T._bwd_case(L, 5, 512, True)
    pa, pb = _run(L, cA, "partials", True, None)[4], _run(L, cB, "partials", True, None)[4]
    assert pa.shape[0] == 3 and pb.shape[0] == 1
    fp = T.Fenced([pa, T._nan(2 * 1024), pb, T._nan(1024)])          # NaN behind each slot's blocks: never read
    fg = T.Fenced([T._t(cA["ca"]), T._t(cA["cb"]), torch.zeros(512), torch.zeros(512)])
    g = [v.data_ptr() for v in fg.views]
    slots = (L.LnSlot * 3)(L.LnSlot(fp.views[0].data_ptr(), 3, g[0], g[1]), L.LnSlot(fp.views[2].data_ptr(), 1, g[0], g[1]),
                           L.LnSlot(fp.views[2].data_ptr(), 1, g[2], g[3]))
    L.check(lib.ortk_ln_partials_reduce(slots, 3, L.stream_ptr()), "ortk_ln_partials_reduce")
    torch.cuda.synchronize()
    assert fp.intact() and fg.intact()
    da, db, da2, db2 = (T._np64(v) for v in fg.views)
    lvA, lvB = _levels(cA["rows"]), _levels(cB["rows"])
    (eaA, taA, ebA, tbA), (eaB, taB, ebB, tbB) = (R.backward_bound(c["dy"].float().numpy(), c["x"], c["a"])[1:] for c in (cA, cB))
    # two atomics per column of the shared destination: the second rounds at |c| + both sums
    ba = R.colsum_bound(eaA, taA, lvA, 1, cA["ca"]) + R.colsum_bound(eaB, taB, lvB, 1, 0) + U * (np.abs(cA["ca"]) + taA + taB)
    bb = R.colsum_bound(ebA, tbA, lvA, 1, cA["cb"]) + R.colsum_bound(ebB, tbB, lvB, 1, 0) + U * (np.abs(cA["cb"]) + tbA + tbB)
    r = (R.ratio(np.abs(da - (cA["ca"] + cA["da"] + cB["da"])), ba), R.ratio(np.abs(db - (cA["cb"] + cA["db"] + cB["db"])), bb),
         R.ratio(np.abs(da2 - cB["da"]), R.colsum_bound(eaB, taB, lvB, 1, 0)), R.ratio(np.abs(db2 - cB["db"]), R.colsum_bound(ebB, tbB, lvB, 1, 0)))
    print(f"ln partials, shared destination: da error / bound {r[0]:.4f}, db {r[1]:.4f}; single slot beside it: da {r[2]:.4f}, db {r[3]:.4f}")
    assert max(r) <= MARGIN


def test_refusals(L):
    """d != 512, an operand off its 16-byte boundary, part or nblocks_out NULL, fewer part_blocks than the launch writes: -1, nothing
    written.  The reduce: a negative count, NULL slots, a slot without a destination."""
    lib, st = L.lib(), L.stream_ptr()
    rows, d = 37, 512
    fin = T.Fenced([torch.ones(rows * d + 8), torch.ones(rows * d), torch.ones(d), torch.ones(rows * 2)])
    fo = T.Fenced([T._nan(rows * d), T._nan(rows * d), T._nan(4 * 2 * d)], torch.float32)
    dy, x, a, s = (L.ptr(v) for v in fin.views)
    dx, dz, part = (L.ptr(v) for v in fo.views)
    nb = C.c_int32(-7)
    call = lambda **k: lib.ortk_layernorm_bwd_part(k.get("dy", dy), 0, k.get("x", x), a, s, None, dx, k.get("part", part), k.get("pb", 4),
                                                   k.get("nb", C.byref(nb)), rows, k.get("d", d), EPS, dz, 0, 0.1, 1, None, st)
    off4 = lambda v: C.c_void_p(v.data_ptr() + 4)
    assert lib.ortk_ln_part_blocks(rows) == 3
    assert call(d=8) == EINVAL and call(d=516) == EINVAL
    assert call(dy=off4(fin.views[0])) == EINVAL and call(part=off4(fo.views[2])) == EINVAL
    assert call(part=None) == EINVAL and call(nb=None) == EINVAL
    assert call(pb=2) == EINVAL
    assert lib.ortk_ln_partials_reduce(None, 1, st) == EINVAL and lib.ortk_ln_partials_reduce(None, -1, st) == EINVAL
    bad = L.LnSlot(fo.views[2].data_ptr(), 1, None, fo.views[0].data_ptr())
    assert lib.ortk_ln_partials_reduce(C.byref(bad), 1, st) == EINVAL
    assert lib.ortk_ln_partials_reduce(None, 0, st) == 0
    torch.cuda.synchronize()
    assert torch.isnan(fo.buf).all() and nb.value == -7
    assert call(pb=3) == 0                           # exactly enough
    torch.cuda.synchronize()
    assert nb.value == 3 and fo.intact() and torch.isnan(fo.views[2][3 * 2 * d:]).all()


# ------------------------------------------------------------------------------------------------ the executor
def _ln_gradients(P, cfgd, b, ln_fuse):
    """loss and every gradient of the second of two mixed-precision XE steps at learning rate 0, under ortk_tuning.ln_fuse"""
    from sparse_image_captioning_amd.training import NativeTrainer
    from sparse_image_captioning_amd.utils.config import Config
    torch.manual_seed(4321)
    m = P.get_model("relation_transformer")(Config(**cfgd), precision="bf16").cuda().eval()
    prev = P._lib.set_tuning(ln_fuse=ln_fuse)
    try:
        tr = NativeTrainer(m, noamopt_factor=0.0, noamopt_warmup=10, keep_grads=True)
        for _ in range(2):
            loss = tr.xe_step(b, train=False)
        torch.cuda.synchronize()
        return loss.clone(), {e["name"]: tr.grads[e["offset"]:e["offset"] + e["numel"]].clone() for e in m.named_weight_entries()}
    finally:
        P._lib.set_tuning(**prev)


@pytest.mark.parametrize("share", [False, True], ids=["plain", "share_dec"])
def test_executor_partials_against_atomics(share):
    """The XE step of the full-width model on the small inputs of the mixed-precision gradient tests, default (partials + one reduce per
    half) against ln_fuse = 16 (atomics): the loss bit-equal, every LayerNorm-parameter gradient at the bar of
    test_mixed_precision_gradients_track_fp32_gradients (cosine > 0.98, relative difference < 0.2).  share_dec:
    three layers, decoder positions 1 and 2 on one module — two slots of one reduce call add into one destination."""
    import common as Cm
    import helpers as H
    import sparse_image_captioning_amd as P
    P._lib.require_gpu()
    cfgd = dict(Cm.FULL_CFG, num_layers=3, share_layer_encoder=(0, 1, 0), share_layer_decoder=(0, 0, 1)) if share else Cm.FULL_CFG
    b = {k: v.cuda() for k, v in H.torch_batch(Cm.make_inputs(**Cm.G2_INPUTS)).items()}
    loss0, g0 = _ln_gradients(P, cfgd, b, 0)
    loss16, g16 = _ln_gradients(P, cfgd, b, 16)
    assert torch.equal(loss0, loss16)
    norms = [n for n in g0 if n.endswith(".a_2") or n.endswith(".b_2")]
    worst = 0.0
    for n in norms:
        a, p = g16[n], g0[n]
        assert float(a.norm()) > 0
        cos = float(torch.dot(a, p) / (a.norm() * p.norm()))
        rel = float((a - p).norm() / a.norm())
        worst = max(worst, rel)
        assert torch.isfinite(p).all() and cos > 0.98 and rel < 0.2, (n, cos, rel)
    print(f"executor, {'shared decoder layers' if share else 'six layers'}: {len(norms)} LayerNorm gradients, largest relative difference {worst:.2e}")
    assert norms and worst < 0.2
