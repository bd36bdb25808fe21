"""ortk_attention_plan — the plan builder of ortk_attention_fwd / ortk_attention_bwd, launching nothing and needing no device — names
the kernel instance, workgroup size and dynamic LDS bytes of every branch of the attention dispatch.  The arguments are made-up
aligned addresses (pointers are tested for alignment only); the expected strings are written out by hand from the dispatch rules and
the LDS figures from the layouts the kernels' comments state."""
import ctypes as C

import pytest

EINVAL, ENOSPC = -1, -2


@pytest.fixture(scope="module")
def L():
    import sparse_image_captioning_amd as P
    P._lib.lib()
    return P._lib


def args(L, Lq, Lk, dk=64, H=8, nkv=4, bwd=False, bf16=False, **kw):
    """AttnArgs over made-up 4 KiB-aligned addresses, packed rows (leading dimensions H * dk); bf16: the mixed-precision step's operands."""
    a = L.AttnArgs()
    a.q, a.k, a.v, a.o, a.p = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    a.nkv, a.H, a.Lq, a.Lk, a.dk = nkv, H, Lq, Lk, dk
    a.ldq = a.ldk = a.ldv = a.ldo = a.lddo = a.lddq = a.lddk = a.lddv = a.ld_new = H * dk
    if bwd:
        a.d_o, a.dq, a.d_k, a.dv, a.dscore = 0x60000, 0x70000, 0x80000, 0x90000, 0xA0000
    if bf16:
        a.precision, a.qkv_dtype, a.o_dtype, a.dqkv_dtype = 1, 1, 1, 1
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


def plan(L, *shape, bwd=False, tuning=None, **kw):
    prev = L.set_tuning(**(tuning or {}))
    try:
        return ";".join(L.attention_plan(args(L, *shape, bwd=bwd, **kw), bwd))
    finally:
        L.set_tuning(**prev)


def code(L, a, bwd=False, tuning=None):
    """The query's return code; a refusal names nothing (the buffer is left as it was)."""
    buf = C.create_string_buffer(b"#" * 64, 64)
    prev = L.set_tuning(**(tuning or {}))
    try:
        e = L.lib().ortk_attention_plan(C.byref(a), int(bwd), buf, 64)
    finally:
        L.set_tuning(**prev)
    assert e == 0 or buf.raw == b"#" * 64
    return e


NEW = dict(k_new=0xB0000, v_new=0xC0000)


# ------------------------------------------------------------------------------------------------ the fp32 family (ortk_attn.hip)
@pytest.mark.parametrize("Lk,inst", [(8, 8), (9, 16), (16, 16), (24, 24), (25, 32), (32, 32)])
def test_rowdec(L, Lk, inst):
    assert plan(L, 1, Lk) == f"rowdec<{inst},f32>:wg=256:lds=0"
    assert plan(L, 1, Lk, kv_dtype=1) == f"rowdec<{inst},bf16>:wg=256:lds=0"
    assert plan(L, 1, Lk, **NEW) == f"rowdec<{inst},f32>:wg=256:lds=0"          # the kernel appends the new key itself
    assert plan(L, 1, Lk, kv_dtype=1, **NEW) == f"rowdec<{inst},bf16>:wg=256:lds=0"


def test_kv_append_then_another_kernel(L):
    assert plan(L, 1, 36, **NEW) == "kv_append:wg=256:lds=0;small_fwd<1,3,f32>:wg=256:lds=0"
    assert plan(L, 1, 36, kv_dtype=1, **NEW) == "kv_append:wg=256:lds=0;small_fwd<1,3,bf16>:wg=256:lds=0"
    assert plan(L, 1, 20, ld_new=8 * 64 + 2, **NEW) == "kv_append:wg=256:lds=0;rowdec<24,f32>:wg=256:lds=0"      # new rows rowdec cannot load by vectors
    assert plan(L, 1, 65, **NEW) == "kv_append:wg=256:lds=0;fwd:wg=256:lds=37384"


@pytest.mark.parametrize("Lk,njt", [(12, 1), (20, 2), (40, 3)])
def test_small_fwd(L, Lk, njt):
    assert plan(L, 12, Lk) == f"small_fwd<1,{njt},f32>:wg=256:lds=0"
    assert plan(L, 20, Lk) == f"small_fwd<2,{njt},f32>:wg=256:lds=0"
    assert plan(L, 12, Lk, kv_dtype=1) == f"small_fwd<1,{njt},bf16>:wg=256:lds=0"
    assert code(L, args(L, 20, Lk, kv_dtype=1)) == EINVAL                      # bf16 K / V: at most 16 query rows


@pytest.mark.parametrize("Lq,Lk,inst", [(12, 12, "1,1"), (12, 20, "1,2"), (20, 12, "2,1"), (20, 20, "2,2")])
def test_small_bwd(L, Lq, Lk, inst):
    assert plan(L, Lq, Lk, bwd=True) == f"small_bwd<{inst}>:wg=256:lds=0"


def test_fwd_mfma(L):
    # lds = 4 (Lkp (66 + 80) + 64 + waves 16 66 2) bytes
    assert plan(L, 36, 36) == "fwd_mfma<48,64>:wg=192:lds=53632"
    assert plan(L, 36, 20) == "fwd_mfma<32,64>:wg=192:lds=44288"
    assert plan(L, 36, 60) == "fwd_mfma<64,64>:wg=192:lds=62976"
    assert plan(L, 36, 36, dk=32) == "fwd_mfma<0,0>:wg=192:lds=53632"
    assert plan(L, 200, 36) == "fwd_mfma<48,64>:wg=512:lds=95872"             # at most 8 waves


def test_bwd_mfma(L):
    # lds = 4 (Lkp 146 + Lqp 278) bytes; part 1: 4 (Lkp 146 + Lqp 132)
    assert plan(L, 36, 36, bwd=True) == "bwd_mfma<48,64,48,0>:wg=192:lds=81408"
    assert plan(L, 85, 36, bwd=True) == "bwd_mfma<48,64,96,0>:wg=384:lds=134784"
    assert plan(L, 85, 36, bwd=True, bwd_part=1) == "bwd_mfma<48,64,96,1>:wg=384:lds=78720"
    assert plan(L, 85, 36, bwd=True, bwd_part=2) == "bwd_mfma<48,64,96,2>:wg=384:lds=134784"
    assert plan(L, 20, 20, bwd=True, tuning=dict(attn_impl=3)) == "bwd_mfma<32,64,32,0>:wg=128:lds=54272"
    assert plan(L, 36, 20, bwd=True) == "bwd_mfma<0,0,0,0>:wg=192:lds=72064"
    assert plan(L, 36, 20, bwd=True, bwd_part=1) == "bwd_mfma<0,0,0,1>:wg=192:lds=44032"
    assert plan(L, 36, 20, bwd=True, bwd_part=2) == "bwd_mfma<0,0,0,2>:wg=192:lds=72064"


def test_wave_kernels_under_attn_impl_1(L):
    t = dict(attn_impl=1)      # lds = 16 (2 Lk 65 + 128 | 192) bytes
    assert plan(L, 17, 17, tuning=t) == "fwd_wave:wg=256:lds=37408"
    assert plan(L, 17, 64, tuning=t) == "fwd_wave:wg=256:lds=135168"
    assert plan(L, 17, 17, bwd=True, tuning=t) == "bwd_wave<32>:wg=256:lds=38432"
    assert plan(L, 17, 40, bwd=True, tuning=t) == "bwd_wave<48>:wg=256:lds=86272"
    assert plan(L, 17, 64, bwd=True, tuning=t) == "bwd_wave<64>:wg=256:lds=136192"
    assert plan(L, 17, 17, bwd=True, bwd_part=2, tuning=t) == ""                # part 1 did everything


def test_decode_under_attn_impl_4(L):
    t = dict(attn_impl=4)
    assert plan(L, 5, 20, tuning=t) == "decode<32>:wg=256:lds=0"
    assert plan(L, 5, 36, tuning=t) == "decode<64>:wg=256:lds=0"
    assert plan(L, 5, 36, drop_p=0.25, tuning=t) == "fwd:wg=256:lds=22304"      # no dropout form: the generic kernel


def test_generic_kernels(L):
    # lds = 4 (2 Lk 65 + 128 + 256 + 512) bytes forward, 4 (4 Lk 65 + 512 + 1024) backward
    assert plan(L, 5, 65, dk=32) == "fwd:wg=256:lds=37384"
    assert plan(L, 5, 65, dk=32, bwd=True) == "bwd:wg=256:lds=73744"
    assert plan(L, 5, 65, dk=32, bwd=True, bwd_part=2) == ""
    assert plan(L, 1, 6, drop_p=0.1, drop_tf_T=17, drop_tf_t=5, drop_tf_lk=17) == "fwd:wg=256:lds=6704"      # (a rowdec shape otherwise)


def test_nothing_to_launch(L):
    assert plan(L, 36, 36, nkv=0) == "" and plan(L, 36, 36, nkv=0, bwd=True) == ""
    assert plan(L, 36, 36, bf16=True, bwd=True, bwd_part=2) == ""              # the bf16-operand kernels do both parts in one


# ------------------------------------------------------------------------------------------------ the bf16-operand family (ortk_attn16.hip)
def test_attn16_short(L):
    # per wave: 6 016 B forward and 9 728 B backward at dk = 64; four waves per workgroup
    assert plan(L, 16, 16, bf16=True) == f"attn16s_fwd<1,64>:wg=256:lds={4 * 6016}"
    assert plan(L, 17, 17, bf16=True) == f"attn16s_fwd<2,64>:wg=256:lds={4 * 6016}"
    assert plan(L, 16, 16, dk=32, bf16=True) == "attn16s_fwd<1,32>:wg=256:lds=15872"
    assert plan(L, 17, 17, dk=32, bf16=True) == "attn16s_fwd<2,32>:wg=256:lds=15872"
    assert plan(L, 16, 16, bf16=True, bwd=True) == f"attn16s_bwd<1,64>:wg=256:lds={4 * 9728}"
    assert plan(L, 17, 17, bf16=True, bwd=True) == f"attn16s_bwd<2,64>:wg=256:lds={4 * 9728}"
    assert plan(L, 16, 16, dk=32, bf16=True, bwd=True) == "attn16s_bwd<1,32>:wg=256:lds=30720"
    assert plan(L, 17, 17, dk=32, bf16=True, bwd=True) == "attn16s_bwd<2,32>:wg=256:lds=30720"


def test_attn16_block(L):
    assert plan(L, 36, 36, bf16=True) == "attn16b_fwd<3,64,1>:wg=192:lds=16384"
    assert plan(L, 85, 36, bf16=True) == "attn16b_fwd<3,64,2>:wg=192:lds=16384"
    assert plan(L, 36, 36, bf16=True, bwd=True) == "attn16b_bwd<3,64,1>:wg=192:lds=27648"
    assert plan(L, 85, 36, bf16=True, bwd=True) == "attn16b_bwd<3,64,2>:wg=192:lds=41472"
    assert plan(L, 33, 33, bf16=True, q_off=0xD0000, q_off_stride=1, kv_ragged=1) == "attn16b_fwd<3,64,1>:wg=192:lds=16384"


def test_attn16_shapes_that_stay_with_the_wave_per_tile_kernels(L):
    BIAS = dict(bias=0xE0000)
    assert plan(L, 36, 100, bf16=True, **BIAS) == "attn16_fwd<7,bf16,64>:wg=192:lds=48128"          # more than 64 keys
    assert plan(L, 36, 100, bf16=True, bwd=True) == "attn16_bwd<7,bf16,64>:wg=192:lds=87808"
    assert plan(L, 97, 36, bf16=True) == "attn16_fwd<3,bf16,64>:wg=448:lds=32768"                   # more than 96 query rows
    assert plan(L, 97, 36, bf16=True, bwd=True) == "attn16_bwd<3,bf16,64>:wg=448:lds=89856"
    assert plan(L, 85, 36, precision=1) == "attn16_fwd<3,f32,64>:wg=384:lds=30464"                  # fp32 Q / K / V
    assert plan(L, 85, 36, precision=1, bwd=True) == "attn16_bwd<3,f32,64>:wg=384:lds=71424"
    assert plan(L, 85, 36, bf16=True, **BIAS) == "attn16_fwd<3,bf16,64>:wg=384:lds=30464"           # a biased block of more than 48 query rows
    assert plan(L, 85, 36, bf16=True, bwd=True, **BIAS) == "attn16_bwd<3,bf16,64>:wg=384:lds=71424"


def test_attn16_min_lq_with_fp32_inputs(L):
    assert plan(L, 33, 36, precision=1) == "attn16_fwd<3,f32,64>:wg=192:lds=23552"
    assert plan(L, 32, 36, precision=1) == "small_fwd<2,3,f32>:wg=256:lds=0"
    assert plan(L, 20, 49, precision=1) == "attn16_fwd<4,f32,64>:wg=128:lds=23552"                  # past 48 keys whatever the row count
    assert plan(L, 20, 48, precision=1) == "small_fwd<2,3,f32>:wg=256:lds=0"
    assert plan(L, 20, 36, precision=1, tuning=dict(attn16_min_lq=20)) == "attn16_fwd<3,f32,64>:wg=128:lds=21248"
    assert plan(L, 32, 36, precision=1, bwd=True) == "bwd_wave<48>:wg=256:lds=77952"
    assert plan(L, 33, 36, precision=1, bwd=True) == "attn16_bwd<3,f32,64>:wg=192:lds=52992"


def test_attn16_switches(L):
    assert plan(L, 17, 17, bf16=True, tuning=dict(attn16_short=0)) == "attn16b_fwd<2,64,1>:wg=192:lds=11776"
    assert plan(L, 17, 17, bf16=True, tuning=dict(attn16_short=1)) == "attn16s_fwd<2,64>:wg=256:lds=24064"
    assert plan(L, 17, 17, bf16=True, tuning=dict(attn16_short=4)) == "attn16s_fwd<2,64>:wg=256:lds=24064"
    assert plan(L, 17, 17, bf16=True, tuning=dict(attn16_short=8)) == "attn16s_fwd<2,64>:wg=512:lds=48128"
    assert plan(L, 17, 17, bf16=True, bwd=True, tuning=dict(attn16_short=8)) == "attn16s_bwd<2,64>:wg=512:lds=77824"
    assert plan(L, 17, 17, bf16=True, tuning=dict(attn16_short=0, attn16_block=0)) == "attn16_fwd<2,bf16,64>:wg=128:lds=14336"
    assert plan(L, 36, 36, bf16=True, tuning=dict(attn16_block=0)) == "attn16_fwd<3,bf16,64>:wg=192:lds=23552"
    assert plan(L, 36, 36, bf16=True, bwd=True, tuning=dict(attn16_block=0)) == "attn16_bwd<3,bf16,64>:wg=192:lds=52992"
    assert plan(L, 36, 36, bf16=True, tuning=dict(attn16_block=1)) == "attn16b_fwd<3,64,1>:wg=192:lds=16384"
    # attn_impl forces the fp32 family only for fp32 operands
    assert plan(L, 85, 36, precision=1, tuning=dict(attn_impl=3)) == "fwd_mfma<48,64>:wg=384:lds=78976"
    assert plan(L, 85, 36, bf16=True, tuning=dict(attn_impl=3)) == "attn16b_fwd<3,64,2>:wg=192:lds=16384"


# ------------------------------------------------------------------------------------------------ refusals and the buffer protocol
def test_refusals(L):
    assert code(L, args(L, 36, 36, qkv_dtype=1)) == EINVAL                                         # bf16 Q / K / V without precision = 1
    assert code(L, args(L, 36, 36, bf16=True, dk=48)) == EINVAL                                    # a head size attn16 does not serve
    assert code(L, args(L, 36, 36, bf16=True, ldq=8 * 64 + 4)) == EINVAL                           # rows not 16-byte aligned
    assert code(L, args(L, 36, 36, precision=1, q_off=0xD0000, q_off_stride=1)) == EINVAL          # ragged groups of fp32 rows
    assert code(L, args(L, 36, 36, bf16=True, q_off=0xD0000, q_off_stride=0)) == EINVAL
    assert code(L, args(L, 36, 36, kv_dtype=1)) == EINVAL                                          # bf16 K / V outside its two kernels
    assert code(L, args(L, 12, 40, kv_dtype=1), tuning=dict(attn_impl=3)) == EINVAL
    assert code(L, args(L, 12, 40, kv_dtype=1, ldk=8 * 64 + 4)) == EINVAL
    assert code(L, args(L, 12, 40, kv_dtype=2)) == EINVAL
    assert code(L, args(L, 12, 12, bwd=True, kv_dtype=1), bwd=True) == EINVAL
    assert code(L, args(L, 1, 20, k_new=0xB0000)) == EINVAL                                        # k_new without v_new
    assert code(L, args(L, 2, 20, **NEW)) == EINVAL                                                # ... with more than one query row
    assert code(L, args(L, 36, 36, bwd=True, bwd_part=3), bwd=True) == EINVAL
    assert code(L, args(L, 36, 36, bf16=True, p=0x50004)) == EINVAL                                # a misaligned p
    assert code(L, args(L, 36, 36, bf16=True, bwd=True, p=0x50004), bwd=True) == EINVAL
    assert code(L, args(L, 36, 36, bwd=True, p=0), bwd=True) == EINVAL
    assert code(L, args(L, 36, 36, bwd=True, kv_group_stride=40), bwd=True) == EINVAL
    assert code(L, args(L, 36, 36, o=0)) == EINVAL and code(L, args(L, 36, 200)) == EINVAL and code(L, args(L, 36, 36, drop_p=1.0)) == EINVAL
    assert code(L, args(L, 1, 6, kv_dtype=1, drop_p=0.1, drop_tf_T=17, drop_tf_lk=17)) == EINVAL   # teacher-forced dropout: fp32 K / V only
    assert L.lib().ortk_attention_plan(None, 0, C.create_string_buffer(8), 8) == EINVAL


def test_buffer_protocol(L):
    lib, a = L.lib(), args(L, 1, 36, kv_dtype=1, **NEW)
    want = b"kv_append:wg=256:lds=0;small_fwd<1,3,bf16>:wg=256:lds=0"
    buf = C.create_string_buffer(b"#" * 80, 80)
    assert lib.ortk_attention_plan(C.byref(a), 0, buf, 8) == ENOSPC and buf.raw == b"#" * 80
    assert lib.ortk_attention_plan(C.byref(a), 0, buf, len(want)) == ENOSPC and buf.raw == b"#" * 80
    assert lib.ortk_attention_plan(C.byref(a), 0, None, 80) == EINVAL and lib.ortk_attention_plan(C.byref(a), 0, buf, 0) == EINVAL
    assert lib.ortk_attention_plan(C.byref(a), 0, buf, len(want) + 1) == 0 and buf.value == want and buf.raw[len(want) + 1:] == b"#" * (79 - len(want))
    a.nkv = 0
    assert lib.ortk_attention_plan(C.byref(a), 0, buf, 1) == 0 and buf.value == b""


def test_lds_figures_of_the_attn16_comments(L):
    """The byte counts the kernels' comments state, from the layouts the kernels carve their LDS by."""
    lds = lambda s: int(s.rsplit("=", 1)[1])
    wg = lambda s: int(s.split(":")[1][3:])
    blk0 = dict(attn16_block=0)
    assert lds(plan(L, 36, 36, bf16=True)) == 16384
    assert [lds(plan(L, q, 36, bf16=True, bwd=True)) for q in (36, 85)] == [27648, 41472]
    s = plan(L, 17, 17, bf16=True, bwd=True)
    assert lds(s) // (wg(s) // 64) == 9728
    s = plan(L, 17, 17, bf16=True)
    assert lds(s) // (wg(s) // 64) == 6016
    assert [lds(plan(L, q, 36, bf16=True, tuning=blk0)) for q in (36, 85)] == [23552, 30464]
    assert [lds(plan(L, q, 36, bf16=True, bwd=True, tuning=blk0)) for q in (36, 85)] == [52992, 71424]
