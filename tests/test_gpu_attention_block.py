"""The second mapping of the bf16-operand block attention kernels of ortk_attn16.hip (attn16b_fwd_kernel / attn16b_bwd_kernel: bf16
Q / K / V / dO, at most 96 query rows and 64 keys per group; three waves per workgroup, up to two query tiles per wave, one shared
image for K, Q and dO in the backward), selected by ortk_tuning.attn16_block.

Every case runs twice through run_case of test_gpu_attention.py — the float64 reference, P == 0 exactly at masked keys, rows of
P summing to 1, NaN sentinels left alone — once with attn16_block = 1 and once with 0, and the two runs must agree BIT FOR BIT on
O, P, dQ, dK, dV and dscore: the new kernels are another mapping of the same per-tile code, not another implementation."""
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


def both_mappings(L, *args, mapped=True, **kw):
    """run_case with attn16_block = 1, then with 0; every output bit-identical.  Returns the first run.  mapped: the shape is one the
    attn16b kernels serve (the plan must name them under 1, and the wave-per-tile kernels under 0 and for every other shape)."""
    old = L.set_tuning(attn16_block=1)
    try:
        out = run_case(L, *args, **kw)
        assert (families(L, out), families(L, out, True)) == ((["attn16b_fwd"], ["attn16b_bwd"]) if mapped else (["attn16_fwd"], ["attn16_bwd"]))
        L.set_tuning(attn16_block=0)
        blk = run_case(L, *args, **kw)
        assert (families(L, blk), families(L, blk, True)) == (["attn16_fwd"], ["attn16_bwd"])
    finally:
        L.set_tuning(attn16_block=old["attn16_block"])
    for name in ("o", "p", "dq", "dk", "dv", "ds"):
        assert torch.equal(bits(out[name]), bits(blk[name])), f"{name}: attn16_block = 1 differs from attn16_block = 0"
    return out


def two_masked(nkv, Lk):
    """Two masked keys (never key 0): the last key of group 0 and key 2 of group 1."""
    km = torch.ones(nkv * Lk); km[Lk - 1] = 0; km[Lk + 2] = 0
    return km


BF16 = dict(precision=1, in_dt=1, out_dt=1)


@pytest.mark.parametrize("dk", [64, 32])
def test_encoder_shape(L, dk):
    """36 x 36 regions with the geometry bias, dscore, two masked keys and probability dropout."""
    nkv, H, S = 3, 4, 36
    both_mappings(L, nkv, H, S, S, dk, use_bias=True, kmask=two_masked(nkv, S), drop_p=0.1, drop_seed=7, **BF16)


@pytest.mark.parametrize("dk", [64, 32])
def test_cross_shape_rectangular(L, dk):
    """85 query rows (six tiles on three waves) against 36 regions, no bias."""
    nkv, H = 2, 4
    both_mappings(L, nkv, H, 85, 36, dk, kmask=two_masked(nkv, 36), drop_p=0.1, drop_seed=9, **BF16)


# captions per image (T = 17, five per image) whose valid rows add up to the group sizes 85, 5, 16, 17, 33 and 64: all six tiles | one
# partial tile | exactly one | a second tile with one row | three tiles, the last with one row (the odd count of a wave that runs two) |
# four full tiles (wave 0 runs two, waves 1 and 2 one)
RAGGED = [17, 17, 17, 17, 17] + [1] * 5 + [4, 4, 4, 3, 1] + [13, 1, 1, 1, 1] + [17, 13, 1, 1, 1] + [17, 17, 17, 12, 1]


@pytest.mark.parametrize("dk", [64, 32])
def test_cross_shape_ragged(L, dk):
    """The valid-position layout: q_off stride 5 (an image's rows are the valid rows of its captions), drop_rows keys the dropout."""
    H, T, spi, Lk = 2, 17, 5, 36
    nimg = len(RAGGED) // spi
    off, row_pos = _caps(RAGGED, T)
    assert [off[(g + 1) * spi] - off[g * spi] for g in range(nimg)] == [85, 5, 16, 17, 33, 64]
    kmask = torch.ones(nimg, Lk); kmask[1, 20:] = 0; kmask[4, 35] = 0
    both_mappings(L, nimg, H, spi * T, Lk, dk, kmask=kmask.view(-1), drop_p=0.1, drop_seed=43, q_off=off, stride=spi, kv_ragged=0,
                  drop_rows=row_pos, poison_p=True, slack=T, **BF16)


def test_cross_shape_ragged_with_an_empty_group(L):
    """q_off[g + 1] == q_off[g]: an image none of whose captions has a valid row (kv_ragged = 0: it still owns 36 keys).  It has no row
    of O, dQ, P or dscore — its blocks of P and dscore keep their NaN sentinels — and its rows of dK and dV are written as zeros."""
    H, T, spi, Lk = 2, 17, 5, 36
    lengths = [17, 17, 17, 17, 17] + [0] * 5 + [4, 4, 4, 3, 1]
    off, row_pos = _caps(lengths, T)
    assert [off[(g + 1) * spi] - off[g * spi] for g in range(3)] == [85, 0, 16]
    kmask = torch.ones(3, Lk); kmask[1, 20:] = 0; kmask[2, 35] = 0
    out = both_mappings(L, 3, H, spi * T, Lk, 64, kmask=kmask.view(-1), drop_p=0.1, drop_seed=43, q_off=off, stride=spi, kv_ragged=0,
                        drop_rows=row_pos, poison_p=True, slack=T, **BF16)
    assert torch.isnan(out["p"][1]).all() and torch.isnan(out["ds"][1]).all()
    assert not out["dk"][Lk:2 * Lk].float().any() and not out["dv"][Lk:2 * Lk].float().any()


@pytest.mark.parametrize("Lk", [33, 37, 48, 64])        # 3 | 3 | 3 | 4 key tiles; 37: P rows not 16-byte aligned
@pytest.mark.parametrize("Lq,bias", [(33, True), (48, True), (49, False), (96, False)])     # 3 tiles | 3 full | 4: two per wave | 6 full
def test_tile_count_edges(L, Lq, Lk, bias):
    nkv, H = 2, 2
    both_mappings(L, nkv, H, Lq, Lk, 64, use_bias=bias, kmask=two_masked(nkv, Lk), drop_p=0.1, drop_seed=11, **BF16)


@pytest.mark.parametrize("Lq,Lk", [(20, 40), (16, 64), (36, 17)])      # Lqp < KJ | one tile, two idle waves | short of 32 keys, past 32 rows
def test_fewer_tiles_than_waves(L, Lq, Lk):
    nkv, H = 2, 2
    both_mappings(L, nkv, H, Lq, Lk, 64, use_bias=True, kmask=two_masked(nkv, Lk), drop_p=0.1, drop_seed=13, **BF16)


def test_ragged_self_attention_of_long_captions(L):
    """kv_ragged = 1 past the short kernels' 32 rows: a group's keys are its own rows (Lkg = Lqg), causal."""
    T, lengths = 40, [40, 33, 7, 17]
    off, _ = _caps(lengths, T)
    both_mappings(L, len(lengths), 2, T, T, 64, causal=T, drop_p=0.1, drop_seed=41, q_off=off, stride=1, kv_ragged=1, poison_p=True,
                  slack=T, **BF16)


@pytest.mark.parametrize("Lq,Lk,in_dt,bias", [
    (36, 100, 1, True),      # more than 64 keys
    (97, 36, 1, False),      # more than 96 query rows
    (85, 36, 0, False),      # fp32 Q / K / V
    (85, 36, 1, True)])      # a biased block of more than 48 query rows
def test_shapes_that_stay_with_the_wave_per_tile_kernels(L, Lq, Lk, in_dt, bias):
    nkv, H = 2, 2
    both_mappings(L, nkv, H, Lq, Lk, 64, use_bias=bias, kmask=two_masked(nkv, Lk), drop_p=0.1, drop_seed=15, precision=1, in_dt=in_dt,
                  out_dt=in_dt, mapped=False)


@pytest.mark.parametrize("with_q_off", [False, True])
@pytest.mark.parametrize("Lq,Lk", [(36, 36), (85, 36)])
def test_dropout_is_the_hash(L, Lq, Lk, with_q_off):
    """The mask the new forward kernel applied, read back through one-hot V rows, is ortk_dropout_apply's.  With q_off the groups are
    all full (the read-back needs the rectangular row order) and drop_rows keys the draws."""
    nkv, H, dk, T, spi = 3, 2, 64, 17, 5
    kw = {}
    if with_q_off:
        if Lq == 85:
            off, row_pos = _caps([T] * (nkv * spi), T)
            kw = dict(q_off=off, stride=spi, drop_rows=row_pos)
        else:
            off, row_pos = _caps([Lq] * nkv, Lq)
            kw = dict(q_off=off, stride=1, drop_rows=row_pos)
    old = L.set_tuning(attn16_block=1)
    try:
        out = run_case(L, nkv, H, Lq, Lk, dk, drop_p=0.3, drop_seed=77, **BF16, **kw)
        assert_mask_is_the_hash(L, out, nkv, H, Lq, Lk, dk, in_dt=1)
    finally:
        L.set_tuning(attn16_block=old["attn16_block"])


def test_switch_values(L):
    old = L.set_tuning()
    assert old["attn16_block"] == 1
    for bad in (-1, 2, 4):
        with pytest.raises(Exception):
            L.set_tuning(attn16_block=bad)
    assert L.set_tuning()["attn16_block"] == 1
