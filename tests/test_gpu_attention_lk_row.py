"""ortk_attention_fwd with per-row key counts (ortk_attn_args.lk_row / kv_index_off: the cached self-attention of rows at different
positions in one launch) against a float64 attention computed group by group, on every kernel that serves one query row per group:
the row kernel (H 8, d_k 64, up to 32 keys), the register-only kernel (33 .. 48 keys in the regular layout), the generic kernel
(everything else, d_k 8 included), each behind kv_append's lk_row instance where it does not append by itself.

Error bars: those of tests/test_gpu_attention.py for the fp32-product kernels on either cache type — assert_close(rtol 1e-4,
atol 2e-5) against float64 computed from the STORED (bf16-rounded) cache values; the new key enters at full precision where the
kernel appends it itself and as the cache stores it where a helper launch appends it first (tests/test_gpu_ops.py::
test_attention_appends_new_key_to_cache).  Without a tolerance: idle groups (0 keys) give all-zero rows, every cache byte outside the
one row an active group appends is unchanged, nothing past a group's key count is read (those table entries point to a NaN row), and
with lk_row = Lk everywhere the call returns the bytes of the call without lk_row."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

NKV, H = 37, 8              # 37 rows: not a multiple of the 4 waves of a row-kernel workgroup
POOL = 64                   # read-only cache rows the ancestry tables may point to
EINVAL = -1


@pytest.fixture(scope="module")
def L():
    import sparse_image_captioning_amd as P
    P._lib.require_gpu()
    return P._lib


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).float()


def bits(t):
    """the tensor's bytes as integers (NaN-safe exact comparison)"""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def draw_lk(Lk, seed):
    """key counts in 0 .. Lk that include 0, 1 and Lk (Lk = 1: both values)"""
    g = torch.Generator().manual_seed(seed)
    lk = torch.randint(0, Lk + 1, (NKV,), generator=g, dtype=torch.int32)
    lk[3], lk[8], lk[NKV - 1] = 0, 1, Lk              # (the last row: the partial workgroup's only wave but one)
    lk[0], lk[20] = Lk, 0
    return lk


def setup(dk, kvdt, Lk, use_idx, lk, seed):
    """Inputs of one case.  Cache: (NKV * T + POOL + 1, d); group g owns rows g T .. g T + T - 1, POOL shared read-only rows follow, the
    last row is NaN.  Without a table the keys of group g are its own rows 0 .. lk - 1.  With one, three blocks of groups have tables
    of their own row stride (as blocks at different positions have): key lk - 1 is a row of the group's own, earlier keys are pool
    rows, entries past lk — and every entry of an idle group — point to the NaN row."""
    d = H * dk
    T = Lk + 3
    tdt = torch.bfloat16 if kvdt else torch.float32
    nrows = NKV * T + POOL + 1
    ck, cv = rnd(nrows, d, seed=seed + 1).to(tdt), rnd(nrows, d, seed=seed + 2).to(tdt)
    ck[-1], cv[-1] = float("nan"), float("nan")
    q, kn, vn = rnd(NKV, d, seed=seed + 3), rnd(NKV, d, seed=seed + 4), rnd(NKV, d, seed=seed + 5)
    keys = []                                                    # physical rows of every group's keys
    table = off = None
    if use_idx:
        g = torch.Generator().manual_seed(seed + 6)
        blocks = ((0, 13), (13, 30), (30, NKV))
        parts, off, base = [], torch.zeros(NKV, dtype=torch.int64), 0
        for bi, (g0, g1) in enumerate(blocks):
            stride = Lk + bi                                     # per-block row stride >= every key count
            t = torch.full((g1 - g0, stride), nrows - 1, dtype=torch.int32)
            for r in range(g1 - g0):
                n = int(lk[g0 + r])
                if n:
                    t[r, :n - 1] = NKV * T + torch.randint(0, POOL, (n - 1,), generator=g, dtype=torch.int32)
                    t[r, n - 1] = (g0 + r) * T + int(torch.randint(0, T, (1,), generator=g))
                    off[g0 + r] = base + r * stride
                else:
                    off[g0 + r] = base + r * stride              # (an idle group's entries are never read: all NaN-row)
            parts.append(t.reshape(-1))
            base += t.numel()
        table = torch.cat(parts)
        for gi in range(NKV):
            keys.append(table[off[gi]:off[gi] + int(lk[gi])].long())
    else:
        for gi in range(NKV):
            keys.append(gi * T + torch.arange(int(lk[gi])))
    return dict(d=d, T=T, ck=ck, cv=cv, q=q, kn=kn, vn=vn, keys=keys, table=table, off=off, tdt=tdt)


def call(L, s, dk, kvdt, Lk, lk):
    """one ortk_attention_fwd on fresh device copies -> (return code, o, cache k, cache v)"""
    dev = lambda t: t.cuda().contiguous()
    qd, knd, vnd, ckd, cvd = dev(s["q"]), dev(s["kn"]), dev(s["vn"]), dev(s["ck"]), dev(s["cv"])
    o = torch.full((NKV, s["d"]), float("nan"), device="cuda")
    a = L.AttnArgs()
    a.q, a.k, a.v, a.o = qd.data_ptr(), ckd.data_ptr(), cvd.data_ptr(), o.data_ptr()
    a.k_new, a.v_new, a.ld_new = knd.data_ptr(), vnd.data_ptr(), s["d"]
    a.ldq = a.ldk = a.ldv = a.ldo = s["d"]
    a.nkv, a.H, a.Lq, a.Lk, a.dk, a.kv_dtype = NKV, H, 1, Lk, dk, kvdt
    hold = [qd, knd, vnd, ckd, cvd]
    if lk is not None:
        lkd = dev(lk); a.lk_row = lkd.data_ptr(); hold.append(lkd)
    if s["table"] is not None:
        td, od = dev(s["table"]), dev(s["off"]); a.kv_index, a.kv_index_off = td.data_ptr(), od.data_ptr(); hold += [td, od]
    else:
        a.kv_group_stride = s["T"]
    plan = ";".join(L.attention_plan(a, False)) if L.lib().ortk_attention_plan(C.byref(a), 0, C.create_string_buffer(256), 256) == 0 else None
    rc = L.lib().ortk_attention_fwd(C.byref(a), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, o.cpu(), ckd.cpu(), cvd.cpu(), plan


@pytest.mark.parametrize("use_idx", [False, True], ids=["stride", "table"])
@pytest.mark.parametrize("Lk", [1, 8, 9, 17, 32, 33, 64])
@pytest.mark.parametrize("kvdt", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("dk", [64, 8])
def test_lk_row_against_float64(L, dk, kvdt, Lk, use_idx):
    lk = draw_lk(Lk, 100 * Lk + dk + kvdt)
    s = setup(dk, kvdt, Lk, use_idx, lk, seed=1000 + 10 * Lk + dk)
    rc, o, ck, cv, plan = call(L, s, dk, kvdt, Lk, lk)
    assert rc == 0 and plan, (rc, plan)
    assert "true>" in plan or "fwd_lk" in plan, plan                          # an lk_row instance served it
    helper = plan.startswith("kv_append_lk")                                  # the new key is read back as the cache stores it
    d, tdt = s["d"], s["tdt"]
    want_k, want_v = s["ck"].clone(), s["cv"].clone()
    for g in range(NKV):
        n = int(lk[g])
        if n:
            row = int(s["keys"][g][n - 1])
            want_k[row], want_v[row] = s["kn"][g].to(tdt), s["vn"][g].to(tdt)
    # ---- exact: the caches differ from their first state in the appended rows alone (idle groups: nowhere), the NaN row included
    assert torch.equal(bits(ck), bits(want_k)), "cache K: a byte outside the appended rows changed"
    assert torch.equal(bits(cv), bits(want_v)), "cache V: a byte outside the appended rows changed"
    # ---- float64 reference, group by group
    ref = torch.zeros(NKV, d, dtype=torch.float64)
    for g in range(NKV):
        n = int(lk[g])
        if n == 0:
            continue
        kk, vv = want_k[s["keys"][g]].double(), want_v[s["keys"][g]].double()
        if not helper:                                                        # appended by the attention kernel: full precision in this step
            kk[n - 1], vv[n - 1] = s["kn"][g].double(), s["vn"][g].double()
        qh, kh, vh = s["q"][g].double().view(H, 1, dk), kk.view(n, H, dk).transpose(0, 1), vv.view(n, H, dk).transpose(0, 1)
        p = torch.softmax(qh @ kh.transpose(1, 2) / dk ** 0.5, -1)
        ref[g] = (p @ vh).reshape(d)
    idle = lk == 0
    assert int(idle.sum()) >= 2
    assert torch.equal(bits(o[idle]), bits(torch.zeros(int(idle.sum()), d))), "an idle group's row is not all zeros"
    assert torch.isfinite(o).all(), "a key past a group's count was read (NaN row) or a row was not written"
    torch.testing.assert_close(o.double(), ref, rtol=1e-4, atol=2e-5)
    # ---- lk_row = Lk everywhere, regular layout: the bytes of the call without lk_row (where that call is served at all)
    if not use_idx:
        full = torch.full((NKV,), Lk, dtype=torch.int32)
        rc_p, o_p, ck_p, cv_p, plan_p = call(L, s, dk, kvdt, Lk, None)
        rc_f, o_f, ck_f, cv_f, plan_f = call(L, s, dk, kvdt, Lk, full)
        assert rc_f == 0
        if rc_p == 0:
            assert torch.equal(bits(o_f), bits(o_p)), ("lk_row = Lk differs from the call without lk_row", plan_f, plan_p)
            assert torch.equal(bits(ck_f), bits(ck_p)) and torch.equal(bits(cv_f), bits(cv_p))
        else:
            # bf16 caches outside the row / register-only kernels' shapes: only the lk_row instance of the generic kernel reads them
            assert rc_p == EINVAL and kvdt == 1 and (dk != 64 or Lk > 48), (rc_p, plan_p)
            assert torch.isfinite(o_f).all()


def test_lk_row_refusals_launch_nothing(L):
    """the refusals of the plan hold for the operator itself: the output keeps its sentinel"""
    lk = draw_lk(17, 5)
    s = setup(64, 0, 17, True, lk, seed=77)
    dev = lambda t: t.cuda().contiguous()
    qd, ckd, cvd, lkd, td = dev(s["q"]), dev(s["ck"]), dev(s["cv"]), dev(lk), dev(s["table"])
    o = torch.full((NKV, s["d"]), float("nan"), device="cuda")
    a = L.AttnArgs()
    a.q, a.k, a.v, a.o, a.lk_row, a.kv_index = qd.data_ptr(), ckd.data_ptr(), cvd.data_ptr(), o.data_ptr(), lkd.data_ptr(), td.data_ptr()
    a.ldq = a.ldk = a.ldv = a.ldo = s["d"]
    a.nkv, a.H, a.Lq, a.Lk, a.dk = NKV, H, 1, 17, 64
    assert L.lib().ortk_attention_fwd(C.byref(a), L.stream_ptr()) == EINVAL        # the table without kv_index_off
    a.kv_index = None
    a.drop_p = 0.1
    assert L.lib().ortk_attention_fwd(C.byref(a), L.stream_ptr()) == EINVAL
    a.drop_p = 0.0
    a.nkv, a.Lq = NKV // 2, 2
    assert L.lib().ortk_attention_fwd(C.byref(a), L.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(o).all()
