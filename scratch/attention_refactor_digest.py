"""SHA-256 of every output array of ortk_attention_fwd / ortk_attention_bwd over the case tables of the three attention test files
(tests/test_gpu_attention.py, test_gpu_attention_short.py, test_gpu_attention_block.py), fixed seeds, through run_case (which also
applies its checks).  One line per case and array: O, P, dQ, dK, dV, dscore.  Run it twice on one build and once on another and diff:
every array the first build reproduces must carry the same digest in the second (profiles/attention_refactor.txt (c)).

    python scratch/attention_refactor_digest.py > digests.txt"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import sparse_image_captioning_amd as P  # noqa: E402
import test_gpu_attention as A  # noqa: E402

L = P._lib
L.require_gpu()
BF16 = dict(precision=1, in_dt=1, out_dt=1)


def two_masked(nkv, Lk):
    km = torch.ones(nkv * Lk); km[Lk - 1] = 0; km[Lk + 2] = 0
    return km


def emit(name, tuning, *args, **kw):
    old = L.set_tuning(**tuning)
    try:
        out = A.run_case(L, *args, **kw)
    finally:
        L.set_tuning(**old)
    tag = ",".join(f"{k}={v}" for k, v in tuning.items()) or "default"
    for k in ("o", "p", "dq", "dk", "dv", "ds"):
        if k in out:
            t = out[k].contiguous()
            raw = t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().tobytes()
            print(f"{name:44s} {tag:32s} {k:3s} {hashlib.sha256(raw).hexdigest()}", flush=True)


def ragged_self(T, dk, lengths, H, tuning, name):
    off, _ = A._caps(lengths, T)
    kmask = torch.ones(off[-1]); kmask[off[0] + min(3, lengths[0] - 1)] = 0
    emit(name, tuning, len(lengths), H, T, T, dk, causal=T, kmask=kmask, drop_p=0.1, drop_seed=41, q_off=off, stride=1, kv_ragged=1,
         poison_p=True, slack=T, **BF16)


def ragged_cross(lengths, sizes, dk, tuning, name):
    H, T, spi, Lk = 2, 17, 5, 36
    off, row_pos = A._caps(lengths, T)
    n = len(lengths) // spi
    assert [off[(g + 1) * spi] - off[g * spi] for g in range(n)] == sizes
    kmask = torch.ones(n, Lk); kmask[1, 20:] = 0; kmask[n - 1, 35] = 0
    emit(name, tuning, n, H, spi * T, Lk, dk, kmask=kmask.view(-1), drop_p=0.1, drop_seed=43, q_off=off, stride=spi, kv_ragged=0,
         drop_rows=row_pos, poison_p=True, slack=T, **BF16)


RAGGED = [17, 17, 17, 17, 17] + [1] * 5 + [4, 4, 4, 3, 1] + [13, 1, 1, 1, 1] + [17, 13, 1, 1, 1] + [17, 17, 17, 12, 1]
EMPTY = [17, 17, 17, 17, 17] + [0] * 5 + [4, 4, 4, 3, 1]

# ---- test_gpu_attention_short.py: both values of attn16_short (and the two explicit widths)
for sw in (1, 0, 4, 8):
    t = dict(attn16_short=sw)
    for T, dk, lengths in [(17, 64, [17, 1, 16, 9, 17, 2, 5]), (25, 32, [25, 3, 16]), (32, 64, [32, 17]), (16, 64, [16, 1]), (16, 32, [16, 1])]:
        ragged_self(T, dk, lengths, 8, t, f"short.ragged T={T} dk={dk}")
    ragged_self(17, 64, [17, 5, 9], 3, t, "short.partly_filled nkv=3 H=3")
    for Lq, Lk in [(20, 20), (9, 30)]:
        emit(f"short.bias_dscore {Lq}x{Lk}", t, 3, 8, Lq, Lk, 64, use_bias=True, kmask=two_masked(3, Lk), drop_p=0.1, drop_seed=3, **BF16)
# ---- test_gpu_attention_block.py: both values of attn16_block
for blk in (1, 0):
    t = dict(attn16_block=blk)
    for dk in (64, 32):
        emit(f"block.encoder dk={dk}", t, 3, 4, 36, 36, dk, use_bias=True, kmask=two_masked(3, 36), drop_p=0.1, drop_seed=7, **BF16)
        emit(f"block.cross dk={dk}", t, 2, 4, 85, 36, dk, kmask=two_masked(2, 36), drop_p=0.1, drop_seed=9, **BF16)
        ragged_cross(RAGGED, [85, 5, 16, 17, 33, 64], dk, t, f"block.cross_ragged dk={dk}")
    for Lk in (33, 37, 48, 64):
        for Lq, bias in [(33, True), (48, True), (49, False), (96, False)]:
            emit(f"block.tile_edges {Lq}x{Lk}", t, 2, 2, Lq, Lk, 64, use_bias=bias, kmask=two_masked(2, Lk), drop_p=0.1, drop_seed=11, **BF16)
    for Lq, Lk in [(20, 40), (16, 64), (36, 17)]:
        emit(f"block.fewer_tiles {Lq}x{Lk}", t, 2, 2, Lq, Lk, 64, use_bias=True, kmask=two_masked(2, Lk), drop_p=0.1, drop_seed=13, **BF16)
    off, _ = A._caps([40, 33, 7, 17], 40)
    emit("block.ragged_self_long", t, 4, 2, 40, 40, 64, causal=40, drop_p=0.1, drop_seed=41, q_off=off, stride=1, kv_ragged=1, poison_p=True,
         slack=40, **BF16)
    for Lq, Lk, in_dt, bias in [(36, 100, 1, True), (97, 36, 1, False), (85, 36, 0, False), (85, 36, 1, True)]:
        emit(f"block.stays {Lq}x{Lk} in_dt={in_dt}", t, 2, 2, Lq, Lk, 64, use_bias=bias, kmask=two_masked(2, Lk), drop_p=0.1, drop_seed=15,
             precision=1, in_dt=in_dt, out_dt=in_dt)
# ---- test_gpu_attention.py: B (short query blocks over more than 64 keys), C (forced families), D (default families), E
for in_dt in (0, 1):
    for nkv, H, Lq, Lk in [(6, 8, 5, 100), (3, 8, 1, 65), (2, 4, 16, 128), (2, 8, 9, 80)]:
        emit(f"B.long_keys {Lq}x{Lk} in_dt={in_dt}", {}, nkv, H, Lq, Lk, 64, kmask=A._tail_mask(nkv, Lk), precision=1, in_dt=in_dt, out_dt=in_dt)
for nkv, H, Lq, Lk, dk, causal, bias, drop in [(3, 8, 17, 17, 64, 17, False, 0.0), (2, 8, 36, 36, 64, 0, True, 0.0), (2, 2, 9, 64, 16, 0, False, 0.0),
                                              (2, 2, 5, 65, 32, 0, False, 0.0), (3, 8, 17, 17, 64, 17, False, 0.3)]:
    emit(f"C.wave {Lq}x{Lk} dk={dk} p={drop}", dict(attn_impl=1), nkv, H, Lq, Lk, dk, causal=causal, use_bias=bias, kmask=A._tail_mask(nkv, Lk),
         drop_p=drop, drop_seed=9)
for nkv, H, Lq, Lk, dk, causal, drop in [(4, 8, 17, 17, 64, 17, 0.0), (2, 8, 12, 40, 64, 0, 0.0), (2, 3, 20, 9, 8, 0, 0.0), (2, 8, 12, 40, 64, 0, 0.3),
                                        (3, 8, 85, 36, 64, 0, 0.1), (2, 4, 20, 20, 16, 0, 0.1)]:
    emit(f"C.fp32_mfma {Lq}x{Lk} dk={dk} p={drop}", dict(attn_impl=3), nkv, H, Lq, Lk, dk, causal=causal, use_bias=True, kmask=A._tail_mask(nkv, Lk),
         drop_p=drop, drop_seed=11)
for nkv, H, Lq, Lk, dk, mask, drop in [(6, 8, 5, 36, 64, True, 0.0), (5, 8, 8, 64, 64, False, 0.0), (7, 8, 1, 33, 64, False, 0.0),
                                      (3, 2, 5, 36, 16, True, 0.0), (4, 8, 4, 20, 64, True, 0.0), (6, 8, 5, 36, 64, True, 0.3)]:
    emit(f"C.decode {Lq}x{Lk} dk={dk} p={drop}", dict(attn_impl=4), nkv, H, Lq, Lk, dk, use_bias=mask, kmask=A._tail_mask(nkv, Lk) if mask else None,
         drop_p=drop, drop_seed=13, bwd=False)
for prec, in_dt in ((0, 0), (1, 0), (1, 1)):      # the default families: register-only, fp32 MFMA, generic; bf16-operand
    for nkv, H, Lq, Lk, dk in [(4, 8, 17, 17, 64), (3, 8, 36, 36, 64), (2, 8, 85, 36, 64), (2, 4, 5, 100, 32), (5, 8, 1, 20, 64)]:
        emit(f"D.default {Lq}x{Lk} dk={dk} prec={prec} in_dt={in_dt}", {}, nkv, H, Lq, Lk, dk, use_bias=Lq == 36, kmask=A._tail_mask(nkv, Lk),
             precision=prec, in_dt=in_dt, out_dt=in_dt, drop_p=0.1, drop_seed=21)
for nkv, Lq, Lk, T, t_, lk in [(12, 1, 6, 17, 5, 17), (4, 5, 36, 17, 3, 36)]:
    emit(f"E.teacher_forced {Lq}x{Lk} t={t_}", {}, nkv, 8, Lq, Lk, 64, kmask=None, drop_p=0.1, drop_seed=17, tf=(T, t_, lk), bwd=False)
# ---- last (a run_case without the empty-group guard stops here): a ragged cross block one of whose groups has no row
for blk in (1, 0):
    ragged_cross(EMPTY, [85, 0, 16], 64, dict(attn16_block=blk), "block.cross_ragged_empty_group")
