"""ortk_attention_fwd / ortk_attention_bwd against one plain float64 attention, at the places the operator tests of
test_gpu_ops.py do not reach: ragged query groups (q_off / kv_ragged / drop_rows), the kernel families that only
ortk_tuning.attn_impl selects, the teacher-forced dropout geometry (drop_tf_*), and the dropout mask itself — replayed from
ortk_dropout_apply over the index space include/ortk.h defines, and recovered from the kernel through one-hot V rows.

Tolerances are the project's: fp32 kernels assert_close(rtol 1e-4, atol 2e-5; saved P atol 1e-5), bf16-operand kernels a max
error below 2 % of the reference tensor's largest magnitude.  Every case also checks what needs no tolerance: P == 0 exactly
at masked / causal-future / not-owned keys, rows of P summing to 1, finite outputs, and NaN sentinels left alone where the
kernel owns nothing."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
EINVAL = -1


@pytest.fixture(scope="module")
def L():
    import sparse_image_captioning_amd as P
    P._lib.require_gpu()
    return P._lib


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).float()


def keep_tensor(L, seed, n, p):
    """0/1 per element of a dropout site of n elements, as the library draws it (ortk_dropout_apply on ones)."""
    ones, out = torch.ones(n, device="cuda"), torch.empty(n, device="cuda")
    L.check(L.lib().ortk_dropout_apply(L.ptr(ones), L.ptr(out), 0, n, p, seed, L.stream_ptr()), "ortk_dropout_apply")
    return (out != 0).double().cpu()


# ------------------------------------------------------------------------------------------------ the reference
def ref_attention(q, k, v, do, qrows, krows, H, dk, kmask=None, bias=None, causal=0, keep=None, p=0.0):
    """Plain float64 attention over per-group row lists.  q / k / v / do: float64 row matrices (H*dk columns); qrows[g] /
    krows[g]: the rows of group g; kmask: one float per row of k; bias[g], keep[g]: (H, nq, nk).  score = q.k/sqrt(dk);
    masked_fill(-1e9) where kmask == 0 or key j > query i % causal; += bias; P = softmax; O = (P * keep / (1-p)) V.
    Returns O (rows of q), P[g] (H, nq, nk), dQ, dK, dV (rows of q / k / v) and dscore[g] for the upstream gradient do."""
    q, k, v = (t.clone().requires_grad_() for t in (q, k, v))
    o = torch.zeros_like(q)
    Ps, Ss = [], []
    for g, (qr, kr) in enumerate(zip(qrows, krows)):
        nq, nk = len(qr), len(kr)
        qh, kh, vh = (t.view(-1, H, dk).transpose(0, 1) for t in (q[qr], k[kr], v[kr]))
        masked = torch.zeros(nq, nk, dtype=torch.bool)
        if kmask is not None:
            masked = masked | (kmask[kr] == 0)[None, :]
        if causal:
            masked = masked | (torch.arange(nk)[None, :] > (torch.arange(nq) % causal)[:, None])
        s = (qh @ kh.transpose(1, 2) / dk ** 0.5).masked_fill(masked[None], -1e9)
        s = s + (bias[g] if bias is not None else 0.0)
        s.retain_grad()
        P = torch.softmax(s, -1)
        Pd = P * keep[g] / (1.0 - p) if keep is not None else P
        o = o.index_add(0, qr, (Pd @ vh).transpose(0, 1).reshape(nq, H * dk))
        Ps.append(P.detach()); Ss.append((s, masked))
    (o * do).sum().backward()
    return {"o": o.detach(), "p": Ps, "masked": [m for _, m in Ss], "dq": q.grad, "dk": k.grad, "dv": v.grad, "ds": [s.grad for s, _ in Ss]}


# ------------------------------------------------------------------------------------------------ one case, end to end
def close(got, want, precision, rtol=1e-4, atol=2e-5, what=""):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), what
    if precision:       # bf16 operands: error relative to the tensor's scale
        err = (got - want).abs().max().item()
        assert err < 2e-2 * max(want.abs().max().item(), 1e-3), (what, err)
    else:
        torch.testing.assert_close(got, want, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


def run_case(L, nkv, H, Lq, Lk, dk, causal=0, use_bias=False, kmask=None, precision=0, in_dt=0, out_dt=0, drop_p=0.0, drop_seed=0,
             q_off=None, stride=1, kv_ragged=0, drop_rows=None, bwd=True, poison_p=False, seed=0, tf=None, slack=0):
    """Run the forward (and backward) of one shape against ref_attention and apply every check of the module docstring.
    q_off (list of ints) selects ragged query groups; kmask is one float per key row; tf = (T, t, lk) the teacher-forced dropout
    geometry; slack = rows of NaN past the last row of every row matrix (a kernel that reads or writes them is caught).
    Returns the kernel's tensors and the reference (for layout-against-layout comparisons)."""
    d = H * dk
    if q_off is None:
        Mq, qrows = nkv * Lq, [torch.arange(g * Lq, (g + 1) * Lq) for g in range(nkv)]
    else:
        Mq, qrows = q_off[-1], [torch.arange(q_off[g * stride], q_off[(g + 1) * stride]) for g in range(nkv)]
    if kv_ragged:
        Mk, krows = Mq, qrows
    else:
        Mk, krows = nkv * Lk, [torch.arange(g * Lk, (g + 1) * Lk) for g in range(nkv)]
    tdt = torch.bfloat16 if in_dt else torch.float32
    odt = torch.bfloat16 if out_dt else torch.float32
    # bf16 storage: the reference computes from the rounded values
    q, k, v, do = (rnd(n, d, seed=seed + s).to(tdt) for n, s in ((Mq, 1), (Mk, 2), (Mk, 3), (Mq, 5)))
    bias = rnd(nkv, H, Lq, Lk, seed=seed + 4) if use_bias else None
    # the keep tensor over the index space of the header
    keep_all = keep_g = None
    if drop_p > 0:
        if tf:
            T, t, lk = tf
            keep_all = keep_tensor(L, drop_seed, nkv * H * Lq * T * lk, drop_p).view(nkv, H, Lq, T, lk)[:, :, :, t, :Lk]
        else:
            keep_all = keep_tensor(L, drop_seed, nkv * H * Lq * Lk, drop_p).view(nkv, H, Lq, Lk)
        keep_g = []
        for g in range(nkv):
            ii = torch.arange(len(qrows[g])) if drop_rows is None else drop_rows[qrows[g]].long() - g * Lq
            keep_g.append(keep_all[g][:, ii, :len(krows[g])])
    ref = ref_attention(q.double(), k.double(), v.double(), do.double(), qrows, krows, H, dk, kmask=kmask,
                        bias=[bias[g, :, :len(qrows[g]), :len(krows[g])].double() for g in range(nkv)] if use_bias else None,
                        causal=causal, keep=keep_g, p=drop_p)

    def rows(t, dtype=None):        # device copy with `slack` NaN rows appended
        pad = torch.full((slack,) + tuple(t.shape[1:]), NAN if t.is_floating_point() else 0, dtype=t.dtype)
        return torch.cat([t, pad]).to(dtype or t.dtype).cuda().contiguous()

    a = L.AttnArgs()
    a.precision, a.qkv_dtype, a.o_dtype, a.dqkv_dtype = precision, in_dt, out_dt, out_dt
    qd, kd, vd, dod = rows(q), rows(k), rows(v), rows(do)
    o = torch.full((Mq + slack, d), NAN, device="cuda", dtype=odt)
    p = torch.full((nkv, H, Lq, Lk), NAN, device="cuda")
    a.q, a.k, a.v, a.o, a.p = qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), p.data_ptr()
    a.ldq = a.ldk = a.ldv = a.ldo = d
    a.nkv, a.H, a.Lq, a.Lk, a.dk, a.causal_period = nkv, H, Lq, Lk, dk, causal
    a.drop_p, a.drop_seed = drop_p, drop_seed
    hold = [qd, kd, vd, dod, o, p]
    if kmask is not None:
        kmd = rows(kmask.float()); a.kmask = kmd.data_ptr(); hold.append(kmd)
    if use_bias:
        bd = bias.cuda(); a.bias = bd.data_ptr(); hold.append(bd)
    if q_off is not None:
        qo = torch.tensor(q_off, dtype=torch.int32).cuda(); hold.append(qo)
        a.q_off, a.q_off_stride, a.kv_ragged = qo.data_ptr(), stride, kv_ragged
    if drop_rows is not None:
        dr = rows(drop_rows.int()); a.drop_rows = dr.data_ptr(); hold.append(dr)
    if tf:
        a.drop_tf_T, a.drop_tf_t, a.drop_tf_lk = tf
    L.check(L.lib().ortk_attention_fwd(C.byref(a), L.stream_ptr()), "attn_fwd")
    torch.cuda.synchronize()
    # ---- forward checks
    oc, pc = o.cpu(), p.cpu()
    close(oc[:Mq], ref["o"], precision, what="O")
    assert torch.isnan(oc[Mq:].float()).all(), "O: rows past the last group were written"
    for g in range(nkv):
        nq, nk = len(qrows[g]), len(krows[g])
        assert torch.isnan(pc[g, :, nq:, :]).all(), f"P[{g}]: rows past the group's count were written"
        if nq == 0:         # (a ragged group without rows: nothing else to compare)
            continue
        blk = pc[g, :, :nq, :]
        close(blk[:, :, :nk], ref["p"][g], precision, atol=1e-5, what=f"P[{g}]")
        assert (blk[:, :, :nk][ref["masked"][g][None].expand(H, -1, -1)] == 0).all(), f"P[{g}]: a masked or causal-future key has P != 0"
        assert (blk[:, :, nk:] == 0).all(), f"P[{g}]: a key the group does not own has P != 0"
        assert (blk.double().sum(-1) - 1).abs().max().item() < 1e-5, f"P[{g}]: rows do not sum to 1"
    out = {"o": oc[:Mq], "p": pc, "ref": ref, "keep": keep_all, "args": a, "hold": hold}
    if not bwd:
        return out
    # ---- backward
    if poison_p:        # the P rows a group does not own are NaN whatever the forward left there: the backward must not read them
        for g in range(nkv):
            p[g, :, len(qrows[g]):, :] = NAN
    dq = torch.full((Mq + slack, d), NAN, device="cuda", dtype=odt)
    dk_, dv = (torch.full((Mk + slack, d), NAN, device="cuda", dtype=odt) for _ in range(2))
    ds = torch.full((nkv, H, Lq, Lk), NAN, device="cuda")
    a.d_o, a.dq, a.d_k, a.dv, a.dscore = dod.data_ptr(), dq.data_ptr(), dk_.data_ptr(), dv.data_ptr(), ds.data_ptr()
    a.lddo = a.lddq = a.lddk = a.lddv = d
    L.check(L.lib().ortk_attention_bwd(C.byref(a), L.stream_ptr()), "attn_bwd")
    torch.cuda.synchronize()
    for name, got, want, n in (("dQ", dq, ref["dq"], Mq), ("dK", dk_, ref["dk"], Mk), ("dV", dv, ref["dv"], Mk)):
        gc = got.cpu()
        close(gc[:n], want, precision, what=name)              # every one of the n rows written (none left NaN), every value right
        assert torch.isnan(gc[n:].float()).all(), f"{name}: rows past the last group were written"
    dsc = ds.cpu()
    for g in range(nkv):
        nq, nk = len(qrows[g]), len(krows[g])
        if nq == 0:
            continue
        close(dsc[g, :, :nq, :nk], ref["ds"][g], precision, what=f"dscore[{g}]")
        assert (dsc[g, :, :nq, nk:] == 0).all(), f"dscore[{g}]: a key the group does not own has a gradient"
    out.update(dq=dq.cpu()[:Mq], dk=dk_.cpu()[:Mk], dv=dv.cpu()[:Mk], ds=dsc)
    return out


def families(L, out, bwd=False):
    """The kernel families ortk_attention_plan names for the arguments of a run_case result, under the tuning values of the moment:
    ["fwd_mfma"], ["attn16b_bwd"], ..."""
    return [k.split(":")[0].split("<")[0] for k in L.attention_plan(out["args"], bwd)]


def recover_keep(L, out, nkv, H, Lq, Lk, dk, in_dt=0):
    """The dropout mask the forward kernel itself applied, read back through one-hot V rows: with V[key j] = e_(j - b*dk) for the
    keys of block b, O[i, h*dk + c] = P[i, b*dk + c] * keep / (1-p) — non-zero exactly where the element was kept (P > 0)."""
    a = out["args"]
    d = H * dk
    got = torch.zeros(nkv, H, Lq, Lk)
    o2 = torch.empty(nkv * Lq, d, device="cuda")
    old = (a.v, a.o, a.o_dtype, a.p)
    for b in range((Lk + dk - 1) // dk):
        v1 = torch.zeros(nkv, Lk, H, dk)
        for j in range(b * dk, min(Lk, (b + 1) * dk)):
            v1[:, j, :, j - b * dk] = 1.0
        v1 = v1.view(nkv * Lk, d).to(torch.bfloat16 if in_dt else torch.float32).cuda()
        a.v, a.o, a.o_dtype, a.p = v1.data_ptr(), o2.data_ptr(), 0, None
        L.check(L.lib().ortk_attention_fwd(C.byref(a), L.stream_ptr()), "attn_fwd")
        torch.cuda.synchronize()
        n = min(Lk, (b + 1) * dk) - b * dk
        got[:, :, :, b * dk:b * dk + n] = (o2.cpu().view(nkv, Lq, H, dk).permute(0, 2, 1, 3)[..., :n] != 0).float()
    a.v, a.o, a.o_dtype, a.p = old
    return got


def assert_mask_is_the_hash(L, out, nkv, H, Lq, Lk, dk, in_dt=0):
    """The mask the kernel applied == the replayed one wherever P > 0 (an element with P == 0 shows nothing), and as many kept."""
    got, want = recover_keep(L, out, nkv, H, Lq, Lk, dk, in_dt), out["keep"].float()
    live = out["p"] > 1e-30
    assert live.float().mean().item() > 0.25
    assert torch.equal(got[live], want[live]), f"{(got[live] != want[live]).sum().item()} of {live.sum().item()} keep decisions differ from the hash"
    assert int(got[live].sum().item()) == int(want[live].sum().item())


# ------------------------------------------------------------------------------------------------ A. ragged query groups
def _caps(lengths, T):
    """Valid-position tables of captions with these lengths: offsets (q_off) and each row's index in the padded (caption, T) layout."""
    off = [0]
    for n in lengths:
        off.append(off[-1] + n)
    row_pos = torch.tensor([c * T + t for c, n in enumerate(lengths) for t in range(n)], dtype=torch.int32)
    return off, row_pos


@pytest.mark.parametrize("T,dk,lengths", [(17, 64, [17, 1, 16, 9, 17, 2, 5]), (25, 32, [25, 3, 16])])
def test_ragged_self_attention(L, T, dk, lengths):
    """The decoder self-attention of the valid-position layout: q_off_stride = 1, kv_ragged = 1 (a caption's keys are its own
    rows; kmask, d_k, dv indexed like q), causal period T, probability dropout on the natural index — forward, backward with the
    not-owned P rows poisoned, and the same captions in the padded rectangular layout under the same seed."""
    H, ncap, p, seed = 8, len(lengths), 0.1, 41
    off, row_pos = _caps(lengths, T)
    Mc = off[-1]
    kmask = torch.ones(Mc); kmask[off[0] + 3] = 0; kmask[off[2] + 7] = 0          # one zero inside two captions
    out = run_case(L, ncap, H, T, T, dk, causal=T, kmask=kmask, precision=1, in_dt=1, out_dt=1, drop_p=p, drop_seed=seed,
                   q_off=off, stride=1, kv_ragged=1, poison_p=True, slack=T)
    # padded layout, same seed: row (c, t) of the rectangle is valid row off[c] + t; pad keys are masked, pad queries are zeros
    d = H * dk
    rp = row_pos.long()
    a = L.AttnArgs()
    qp, kp, vp = (torch.zeros(ncap * T, d, dtype=torch.bfloat16) for _ in range(3))
    for dst, s in ((qp, 1), (kp, 2), (vp, 3)):
        dst[rp] = rnd(Mc, d, seed=s).bfloat16()
    kmp = torch.zeros(ncap * T); kmp[rp] = kmask
    qd, kd, vd, kmd = qp.cuda(), kp.cuda(), vp.cuda(), kmp.cuda()
    o = torch.full((ncap * T, d), NAN, device="cuda", dtype=torch.bfloat16)
    a.precision, a.qkv_dtype, a.o_dtype = 1, 1, 1
    a.q, a.k, a.v, a.o, a.kmask = qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), kmd.data_ptr()
    a.ldq = a.ldk = a.ldv = a.ldo = d
    a.nkv, a.H, a.Lq, a.Lk, a.dk, a.causal_period, a.drop_p, a.drop_seed = ncap, H, T, T, dk, T, p, seed
    L.check(L.lib().ortk_attention_fwd(C.byref(a), L.stream_ptr()), "attn_fwd")
    close(o.cpu()[rp], out["o"].double(), 1, what="O: padded layout against the valid-position layout")
    close(o.cpu()[rp], out["ref"]["o"], 1, what="O: padded layout against the reference")


@pytest.mark.parametrize("Lk", [36, 100])
def test_ragged_cross_attention(L, Lk):
    """The decoder cross-attention of the valid-position layout: q_off_stride = captions per image (an image's query rows are
    the valid rows of its captions), rectangular keys, drop_rows = each row's padded index so the dropout is the padded
    layout's.  Lk = 100 is the 7-key-tile instance with the 136-element image pitch."""
    H, dk, T, spi, nimg, p, seed = 8, 64, 17, 5, 3, 0.1, 43
    lengths = [17, 4, 9, 1, 12] + [1] * 5 + [17] * 5             # mixed | five rows: one partial tile | all 85 rows
    off, row_pos = _caps(lengths, T)
    Mc, Lq, d = off[-1], spi * T, H * dk
    kmask = torch.ones(nimg, Lk); kmask[1, 20:] = 0              # image 1 has 20 regions
    out = run_case(L, nimg, H, Lq, Lk, dk, kmask=kmask.view(-1), precision=1, in_dt=1, out_dt=1, drop_p=p, drop_seed=seed,
                   q_off=off, stride=spi, kv_ragged=0, drop_rows=row_pos, poison_p=True, slack=T)
    # padded layout, same seed (run_case draws K / V from the same seeds; the pad queries are zeros)
    rp = row_pos.long()
    a = L.AttnArgs()
    qp = torch.zeros(nimg * Lq, d, dtype=torch.bfloat16); qp[rp] = rnd(Mc, d, seed=1).bfloat16()
    qd, kd, vd, kmd = qp.cuda(), rnd(nimg * Lk, d, seed=2).bfloat16().cuda(), rnd(nimg * Lk, d, seed=3).bfloat16().cuda(), kmask.cuda()
    o = torch.full((nimg * Lq, d), NAN, device="cuda", dtype=torch.bfloat16)
    a.precision, a.qkv_dtype, a.o_dtype = 1, 1, 1
    a.q, a.k, a.v, a.o, a.kmask = qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), kmd.data_ptr()
    a.ldq = a.ldk = a.ldv = a.ldo = d
    a.nkv, a.H, a.Lq, a.Lk, a.dk, a.drop_p, a.drop_seed = nimg, H, Lq, Lk, dk, p, seed
    L.check(L.lib().ortk_attention_fwd(C.byref(a), L.stream_ptr()), "attn_fwd")
    close(o.cpu()[rp], out["o"].double(), 1, what="O: padded layout against the valid-position layout")
    close(o.cpu()[rp], out["ref"]["o"], 1, what="O: padded layout against the reference")


def test_ragged_groups_are_refused_outside_the_bf16_operand_kernels(L):
    H, dk, T = 8, 64, 17
    off = torch.tensor([0, 17, 20], dtype=torch.int32).cuda()
    for qkv_dtype, precision, stride in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        tdt = torch.bfloat16 if qkv_dtype else torch.float32
        t = torch.zeros(2 * T, H * dk, device="cuda", dtype=tdt); o = torch.zeros(2 * T, H * dk, device="cuda")
        a = L.AttnArgs()
        a.q = a.k = a.v = t.data_ptr(); a.o = o.data_ptr(); a.ldq = a.ldk = a.ldv = a.ldo = H * dk
        a.nkv, a.H, a.Lq, a.Lk, a.dk = 2, H, T, T, dk
        a.qkv_dtype, a.precision, a.q_off, a.q_off_stride, a.kv_ragged = qkv_dtype, precision, off.data_ptr(), stride, 1
        assert L.lib().ortk_attention_fwd(C.byref(a), L.stream_ptr()) == EINVAL, (qkv_dtype, precision, stride)
        p = torch.zeros(2, H, T, T, device="cuda")
        a.p = p.data_ptr(); a.d_o = t.data_ptr(); a.dq = a.d_k = a.dv = o.data_ptr(); a.lddo = a.lddq = a.lddk = a.lddv = H * dk
        assert L.lib().ortk_attention_bwd(C.byref(a), L.stream_ptr()) == EINVAL, (qkv_dtype, precision, stride)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ B. one wave, more than 64 keys
@pytest.mark.parametrize("in_dt", [0, 1])
@pytest.mark.parametrize("nkv,H,Lq,Lk", [(6, 8, 5, 100), (3, 8, 1, 65), (2, 4, 16, 128), (2, 8, 9, 80)])
def test_short_query_blocks_over_more_than_64_keys(L, nkv, H, Lq, Lk, in_dt):
    """At most 16 query rows launch ONE wave of the bf16-operand forward; its key mask has 128 entries.  Group g keeps keys
    [0, 40 + g) and [70, 90): a masked run that starts below key 64 and one above it.  What decides it is P == 0 exactly at the
    masked keys >= 64 (run_case asserts it for every masked key)."""
    kmask = torch.zeros(nkv, Lk)
    for g in range(nkv):
        kmask[g, :40 + g] = 1; kmask[g, 70:90] = 1
    assert (kmask[:, 64:] == 0).any()
    run_case(L, nkv, H, Lq, Lk, 64, kmask=kmask.view(-1), precision=1, in_dt=in_dt, out_dt=in_dt)


# ------------------------------------------------------------------------------------------------ C. forced kernel families
class forced:
    def __init__(self, L, impl):
        self.L, self.impl = L, impl

    def __enter__(self):
        self.old = self.L.set_tuning(attn_impl=self.impl)

    def __exit__(self, *exc):
        self.L.set_tuning(attn_impl=self.old["attn_impl"])


def _tail_mask(nkv, Lk):
    """group g loses its last 1 + g keys (never key 0)"""
    km = torch.ones(nkv, Lk)
    for g in range(nkv):
        km[g, max(1, Lk - 1 - g):] = 0
    return km.view(-1)


@pytest.mark.parametrize("nkv,H,Lq,Lk,dk,causal,bias,drop", [
    (3, 8, 17, 17, 64, 17, False, 0.0),
    (2, 8, 36, 36, 64, 0, True, 0.0),
    (2, 2, 9, 64, 16, 0, False, 0.0),        # Lk = 64: the last key count of the wave kernels; dk = 16: scalar loads
    (2, 2, 5, 65, 32, 0, False, 0.0),        # one key too many: the generic kernels
    (3, 8, 17, 17, 64, 17, False, 0.3)])
def test_wave_kernels(L, nkv, H, Lq, Lk, dk, causal, bias, drop):
    """attn_impl = 1: attn_fwd_wave_kernel and attn_bwd_wave_kernel<32 | 48 | 64>."""
    with forced(L, 1):
        out = run_case(L, nkv, H, Lq, Lk, dk, causal=causal, use_bias=bias, kmask=_tail_mask(nkv, Lk), drop_p=drop, drop_seed=9)
        assert families(L, out) == (["fwd_wave"] if Lk <= 64 else ["fwd"]) and families(L, out, True) == (["bwd_wave"] if Lk <= 64 else ["bwd"])
        if drop:
            assert_mask_is_the_hash(L, out, nkv, H, Lq, Lk, dk)


@pytest.mark.parametrize("nkv,H,Lq,Lk,dk,causal,drop", [
    (4, 8, 17, 17, 64, 17, 0.0),
    (2, 8, 12, 40, 64, 0, 0.0),              # 48 padded keys: the <48, 64> forward instance
    (2, 3, 20, 9, 8, 0, 0.0),                # dk padded to 16: the general <0, 0> instances
    (2, 8, 12, 40, 64, 0, 0.3)])
def test_fp32_mfma_kernels_on_short_query_blocks(L, nkv, H, Lq, Lk, dk, causal, drop):
    """attn_impl = 3: the fp32-MFMA block kernels below their automatic threshold of 33 query rows."""
    with forced(L, 3):
        out = run_case(L, nkv, H, Lq, Lk, dk, causal=causal, use_bias=True, kmask=_tail_mask(nkv, Lk), drop_p=drop, drop_seed=11)
        assert families(L, out) == ["fwd_mfma"] and families(L, out, True) == ["bwd_mfma"]
        if drop:
            assert_mask_is_the_hash(L, out, nkv, H, Lq, Lk, dk)


@pytest.mark.parametrize("nkv,H,Lq,Lk,dk", [(3, 8, 85, 36, 64), (2, 4, 20, 20, 16)])
def test_fp32_mfma_backward_in_two_parts(L, nkv, H, Lq, Lk, dk):
    """attn_impl = 3: bwd_part 1 then 2 == bwd_part 0 bit for bit (the <48, 64, 96, 1 | 2> and the general <0, 0, 0, 1 | 2> instances),
    and bwd_part 0 is right."""
    with forced(L, 3):
        out = run_case(L, nkv, H, Lq, Lk, dk, use_bias=True, kmask=_tail_mask(nkv, Lk), drop_p=0.1, drop_seed=5)
        a = out["args"]
        d = H * dk
        dq, dk_, dv = (torch.full((n, d), NAN, device="cuda") for n in (nkv * Lq, nkv * Lk, nkv * Lk))
        ds = torch.full((nkv, H, Lq, Lk), NAN, device="cuda")
        a.dq, a.d_k, a.dv, a.dscore = dq.data_ptr(), dk_.data_ptr(), dv.data_ptr(), ds.data_ptr()
        assert families(L, out, True) == ["bwd_mfma"]
        for part in (1, 2):
            a.bwd_part = part
            assert families(L, out, True) == ["bwd_mfma"]
            L.check(L.lib().ortk_attention_bwd(C.byref(a), L.stream_ptr()), "attn_bwd")
            if part == 1:       # part 1 guarantees dQ and dscore
                torch.cuda.synchronize()
                assert torch.equal(dq.cpu(), out["dq"]) and torch.equal(ds.cpu(), out["ds"])
        torch.cuda.synchronize()
        for name, got in (("dq", dq), ("dk", dk_), ("dv", dv), ("ds", ds)):
            assert torch.equal(got.cpu(), out[name]), name


@pytest.mark.parametrize("nkv,H,Lq,Lk,dk,mask,drop", [
    (6, 8, 5, 36, 64, True, 0.0),            # attn_decode_kernel<64>
    (5, 8, 8, 64, 64, False, 0.0),           # most query rows, most keys
    (7, 8, 1, 33, 64, False, 0.0),
    (3, 2, 5, 36, 16, True, 0.0),
    (4, 8, 4, 20, 64, True, 0.0),            # attn_decode_kernel<32>
    (6, 8, 5, 36, 64, True, 0.3)])           # no dropout form: whichever kernel serves the shape (the generic one)
def test_decode_kernel(L, nkv, H, Lq, Lk, dk, mask, drop):
    """attn_impl = 4: attn_decode_kernel<32 | 64> (forward only; up to 8 query rows, 64 keys, no causal mask, no dropout)."""
    with forced(L, 4):
        out = run_case(L, nkv, H, Lq, Lk, dk, use_bias=mask, kmask=_tail_mask(nkv, Lk) if mask else None, drop_p=drop, drop_seed=13, bwd=False)
        assert families(L, out) == (["fwd"] if drop else ["decode"])
        if drop:
            assert_mask_is_the_hash(L, out, nkv, H, Lq, Lk, dk)


# ------------------------------------------------------------------------------------------------ D. dropout replay
@pytest.mark.parametrize("drop", [0.1, 0.3])
@pytest.mark.parametrize("nkv,H,Lq,Lk,dk,prec,in_dt,bias", [
    (5, 8, 17, 17, 64, 0, 0, False),         # register-only small kernels
    (4, 8, 20, 9, 64, 0, 0, True),
    (2, 8, 36, 36, 64, 0, 0, True),          # fp32-MFMA
    (2, 8, 85, 36, 64, 0, 0, False),
    (2, 2, 5, 100, 32, 0, 0, False),         # generic
    (2, 8, 36, 36, 64, 1, 1, True),          # bf16-operand
    (2, 8, 85, 36, 64, 1, 1, False),
    (2, 4, 40, 13, 64, 1, 0, False)])        # Lk not a multiple of 4: a group of four keep decisions straddles the row end
def test_dropout_is_the_hash_on_every_default_family(L, nkv, H, Lq, Lk, dk, prec, in_dt, bias, drop):
    """Element ((g*H + h)*Lq + i)*Lk + j of the site keeps iff ortk_dropout_apply(ones, ..)[that index] != 0: O, dQ, dK, dV and
    dscore equal the float64 attention under exactly that mask, and the mask read back from the kernel is that mask."""
    out = run_case(L, nkv, H, Lq, Lk, dk, causal=17 if Lq == Lk == 17 else 0, use_bias=bias, kmask=_tail_mask(nkv, Lk), precision=prec,
                   in_dt=in_dt, drop_p=drop, drop_seed=77)
    rate = out["keep"].mean().item()
    assert abs(rate - (1 - drop)) < 5 * (drop * (1 - drop) / out["keep"].numel()) ** 0.5 + 1.0 / 65536     # the hash itself: 5 sigma
    assert_mask_is_the_hash(L, out, nkv, H, Lq, Lk, dk, in_dt)


# ------------------------------------------------------------------------------------------------ E. teacher-forced dropout geometry
@pytest.mark.parametrize("nkv,Lq,Lk,T,t,lk", [(12, 1, 1, 17, 0, 17), (12, 1, 6, 17, 5, 17), (12, 1, 17, 17, 16, 17),      # self-attention step t
                                              (4, 5, 36, 17, 3, 36)])                                                   # cross-attention step
def test_teacher_forced_dropout_geometry(L, nkv, Lq, Lk, T, t, lk):
    """drop_tf_T / drop_tf_t / drop_tf_lk: a decode step at position t draws element
    ((g*H + h)*(Lq*T) + i*T + t)*lk + j of the teacher-forced pass's site (generic kernel, precision 0)."""
    H, dk = 8, 64
    out = run_case(L, nkv, H, Lq, Lk, dk, drop_p=0.3, drop_seed=21, tf=(T, t, lk), bwd=False,
                   kmask=_tail_mask(nkv, Lk) if Lk == 36 else None)
    assert_mask_is_the_hash(L, out, nkv, H, Lq, Lk, dk)


def test_teacher_forced_dropout_is_refused_with_bf16_kv(L):
    H, dk, nkv, Lk = 8, 64, 4, 13
    q, o = torch.zeros(nkv, H * dk, device="cuda"), torch.zeros(nkv, H * dk, device="cuda")
    kv = torch.zeros(nkv * Lk, H * dk, device="cuda", dtype=torch.bfloat16)
    a = L.AttnArgs()
    a.q, a.k, a.v, a.o = q.data_ptr(), kv.data_ptr(), kv.data_ptr(), o.data_ptr()
    a.ldq = a.ldk = a.ldv = a.ldo = H * dk
    a.nkv, a.H, a.Lq, a.Lk, a.dk, a.kv_dtype = nkv, H, 1, Lk, dk, 1
    a.drop_p, a.drop_seed, a.drop_tf_T, a.drop_tf_t, a.drop_tf_lk = 0.3, 1, 17, 12, 17
    assert L.lib().ortk_attention_fwd(C.byref(a), L.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
