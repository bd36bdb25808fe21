"""The one-wave-per-(group, head) attention kernels of ortk_attn16.hip (attn16s_fwd_kernel / attn16s_bwd_kernel: bf16 Q / K / V / dO,
at most 32 query rows and 32 keys per group), selected by ortk_tuning.attn16_short.

Every case runs twice through run_case of test_gpu_attention.py — the float64 reference, P == 0 exactly at masked keys, rows of
P summing to 1, NaN sentinels left alone — once with the switch on and once with attn16_short = 0, and the two runs must agree
BIT FOR BIT on O, P, dQ, dK, dV and dscore: the short kernels are a second mapping of the same per-tile code, not a second
implementation."""
import pytest
import torch

from test_gpu_attention import run_case, _caps, assert_mask_is_the_hash, families, rnd  # noqa: F401  (rnd: the operands run_case draws)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import sparse_image_captioning_amd as P
    P._lib.require_gpu()
    return P._lib


def bits(t):
    """The tensor's bit patterns (NaN sentinels compare equal)."""
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def short_and_block(L, *args, short=1, **kw):
    """run_case with attn16_short = `short`, then with 0; every output bit-identical.  Returns the first run."""
    old = L.set_tuning(attn16_short=short)
    try:
        out = run_case(L, *args, **kw)
        assert families(L, out) == ["attn16s_fwd"] and ("dq" not in out or families(L, out, True) == ["attn16s_bwd"])
        L.set_tuning(attn16_short=0)
        blk = run_case(L, *args, **kw)
        assert families(L, blk)[0] in ("attn16_fwd", "attn16b_fwd") and ("dq" not in blk or families(L, blk, True)[0] in ("attn16_bwd", "attn16b_bwd"))
    finally:
        L.set_tuning(attn16_short=old["attn16_short"])
    for name in ("o", "p", "dq", "dk", "dv", "ds"):
        if name in out:
            assert torch.equal(bits(out[name]), bits(blk[name])), f"{name}: attn16_short = {short} differs from the block kernels"
    return out


def ragged(L, T, dk, lengths, H=8, short=1, zero_key=True, p=0.1):
    """The decoder self-attention of the valid-position layout (test_ragged_self_attention), through both kernel mappings."""
    off, _ = _caps(lengths, T)
    kmask = torch.ones(off[-1])
    if zero_key:
        kmask[off[0] + min(3, lengths[0] - 1)] = 0          # one zero inside the first caption (never its key 0)
    return short_and_block(L, len(lengths), H, T, T, dk, causal=T, kmask=kmask, precision=1, in_dt=1, out_dt=1, drop_p=p, drop_seed=41,
                           q_off=off, stride=1, kv_ragged=1, poison_p=True, slack=T, short=short)


@pytest.mark.parametrize("T,dk,lengths", [
    (17, 64, [17, 1, 16, 9, 17, 2, 5]),      # tile 1: one row | absent | empty
    (25, 32, [25, 3, 16]),
    (32, 64, [32, 17]),                      # both tiles full
    (16, 64, [16, 1]),                       # exactly one tile
    (16, 32, [16, 1])])
def test_ragged_causal_self_attention(L, T, dk, lengths):
    ragged(L, T, dk, lengths)


def test_one_position(L):
    """T = 1: one query, one key (no key to mask: a caption's only key stays)."""
    ragged(L, 1, 64, [1, 1, 1], zero_key=False)


@pytest.mark.parametrize("nkv,H,lengths,short", [
    (3, 2, [17, 9, 3], 1),                   # 6 pairs: not a multiple of 4
    (3, 2, [17, 9, 3], 4),
    (3, 2, [17, 9, 3], 8),                   # ... nor of 8
    (5, 4, [17, 1, 16, 9, 5], 8)])           # 20 pairs, 8 waves per workgroup: the last workgroup holds 4
def test_partly_filled_last_workgroup(L, nkv, H, lengths, short):
    ragged(L, 17, 64, lengths, H=H, short=short)


@pytest.mark.parametrize("with_drop_rows", [False, True])
def test_rectangular_layout(L, with_drop_rows):
    """No q_off: every group holds Lq rows; drop_rows (each row's own index: what the padded layout's table says) changes nothing."""
    nkv, H, T = 3, 8, 17
    _, row_pos = _caps([T] * nkv, T)
    kmask = torch.ones(nkv * T); kmask[T + 5] = 0
    short_and_block(L, nkv, H, T, T, 64, causal=T, kmask=kmask, precision=1, in_dt=1, out_dt=1, drop_p=0.1, drop_seed=41,
                    drop_rows=row_pos if with_drop_rows else None)


@pytest.mark.parametrize("Lq,Lk", [(20, 20), (9, 30)])       # (9, 30): one query tile, two key tiles, P rows not 16-byte aligned
def test_short_block_with_bias_and_dscore(L, Lq, Lk):
    nkv, H = 2, 4
    kmask = torch.ones(nkv * Lk); kmask[Lk - 1] = 0; kmask[Lk + 2] = 0
    short_and_block(L, nkv, H, Lq, Lk, 64, use_bias=True, kmask=kmask, precision=1, in_dt=1, out_dt=1, drop_p=0.1, drop_seed=7)


@pytest.mark.parametrize("drop", [0.1, 0.3])
@pytest.mark.parametrize("with_q_off", [False, True])
def test_dropout_is_the_hash(L, drop, with_q_off):
    """The mask the short forward kernel applied, read back through one-hot V rows, is ortk_dropout_apply's.  With q_off the captions
    are all full (the read-back needs the rectangular row order) and drop_rows keys the draws."""
    nkv, H, T, dk = 3, 8, 17, 64
    off, row_pos = _caps([T] * nkv, T)
    kw = dict(q_off=off, stride=1, kv_ragged=1, drop_rows=row_pos) if with_q_off else {}
    old = L.set_tuning(attn16_short=1)
    try:
        out = run_case(L, nkv, H, T, T, dk, causal=T, precision=1, in_dt=1, out_dt=1, drop_p=drop, drop_seed=77, **kw)
        assert_mask_is_the_hash(L, out, nkv, H, T, T, dk, in_dt=1)
    finally:
        L.set_tuning(attn16_short=old["attn16_short"])


def test_switch_values(L):
    old = L.set_tuning()
    assert old["attn16_short"] == 1
    for bad in (-1, 2, 3, 16):
        with pytest.raises(Exception):
            L.set_tuning(attn16_short=bad)
    assert L.set_tuning()["attn16_short"] == 1
