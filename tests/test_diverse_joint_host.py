"""The joint diverse executor (ORTK_DEC_GROUPS_JOINT, `executor="unfused_joint"`), CPU side — no device:
  * ortk_attention_plan with per-row key counts (ortk_attn_args.lk_row / kv_index_off): the routing to the kernels' lk_row instances
    and every refusal;
  * ortk_decode_workspace_bytes with the joint flag: what it adds and what it refuses;
  * the option parsing: `executor="unfused_joint"` and its refusals, each naming its reason;
  * the restatement on the inputs of the edge-schedule cases of tests/test_gpu_diverse_joint.py: enough images with a decision margin."""
import ctypes as Ct

import pytest
import torch

import common as C
import diverse_beam_ref as D
import diverse_joint_cases as J
import helpers as H
from oracle import ort_oracle as O

EINVAL = -1
LK_ROW, KV_OFF, KV_INDEX = 0xD0000, 0xE0000, 0xF0000       # made-up aligned addresses: the plan only tests pointers for alignment
NEW = dict(k_new=0xB0000, v_new=0xC0000)


@pytest.fixture(scope="module")
def L():
    import sparse_image_captioning_amd as P
    P._lib.lib()
    return P._lib


def args(L, Lq, Lk, dk=64, H=8, nkv=37, **kw):
    a = L.AttnArgs()
    a.q, a.k, a.v, a.o = 0x10000, 0x20000, 0x30000, 0x40000
    a.nkv, a.H, a.Lq, a.Lk, a.dk = nkv, H, Lq, Lk, dk
    a.ldq = a.ldk = a.ldv = a.ldo = a.lddo = a.lddq = a.lddk = a.lddv = a.ld_new = H * dk
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


def plan(L, *shape, bwd=False, **kw):
    return ";".join(L.attention_plan(args(L, *shape, **kw), bwd))


def code(L, a, bwd=False):
    buf = Ct.create_string_buffer(b"#" * 96, 96)
    e = L.lib().ortk_attention_plan(Ct.byref(a), int(bwd), buf, 96)
    assert e == 0 or buf.raw == b"#" * 96          # a refusal names nothing
    return e


# ------------------------------------------------------------------------------------------------ attention plan
def test_struct_mirror_ends_with_the_new_fields(L):
    names = [f[0] for f in L.AttnArgs._fields_]
    assert names[-2:] == ["lk_row", "kv_index_off"]
    assert L.ABI_VERSION == L.lib().ortk_version()


@pytest.mark.parametrize("kv_dtype,kvt", [(0, "f32"), (1, "bf16")])
def test_lk_row_plan_row_kernel(L, kv_dtype, kvt):
    """H 8, d_k 64, Lk 17: the row kernel's lk_row instance, with and without the ancestry table, appending by itself"""
    assert plan(L, 1, 17, kv_dtype=kv_dtype, lk_row=LK_ROW) == f"rowdec<24,{kvt},true>:wg=256:lds=0"
    assert plan(L, 1, 17, kv_dtype=kv_dtype, lk_row=LK_ROW, **NEW) == f"rowdec<24,{kvt},true>:wg=256:lds=0"
    assert plan(L, 1, 17, kv_dtype=kv_dtype, lk_row=LK_ROW, kv_index=KV_INDEX, kv_index_off=KV_OFF, **NEW) == f"rowdec<24,{kvt},true>:wg=256:lds=0"
    assert plan(L, 1, 17, kv_dtype=kv_dtype) == f"rowdec<24,{kvt}>:wg=256:lds=0"          # (the call without: the instance it always took)


def test_lk_row_plan_generic_and_register_kernels(L):
    # d_k 8 (the tiny golden model): the generic kernel, behind the append; lds = 4 (2 Lk 65 + 128 + 4 64 + 4 128) bytes
    assert plan(L, 1, 17, dk=8, lk_row=LK_ROW) == "fwd_lk:wg=256:lds=12424"
    assert plan(L, 1, 17, dk=8, lk_row=LK_ROW, kv_index=KV_INDEX, kv_index_off=KV_OFF, **NEW) == "kv_append_lk:wg=256:lds=0;fwd_lk:wg=256:lds=12424"
    assert plan(L, 1, 17, dk=8, **NEW) == "kv_append:wg=256:lds=0;fwd:wg=256:lds=12424"
    # 33 .. 48 keys in the regular layout: the register-only kernel, as without lk_row; with the table, or past 48 keys: the generic one
    assert plan(L, 1, 33, lk_row=LK_ROW) == "small_fwd<1,3,f32,true>:wg=256:lds=0"
    assert plan(L, 1, 33, kv_dtype=1, lk_row=LK_ROW, **NEW) == "kv_append_lk:wg=256:lds=0;small_fwd<1,3,bf16,true>:wg=256:lds=0"
    assert plan(L, 1, 33, lk_row=LK_ROW, kv_index=KV_INDEX, kv_index_off=KV_OFF) == "fwd_lk:wg=256:lds=20744"
    assert plan(L, 1, 64, lk_row=LK_ROW) == "fwd_lk:wg=256:lds=36864"
    # bf16 caches where no other kernel reads them: the generic kernel's lk_row instance does
    assert plan(L, 1, 64, kv_dtype=1, lk_row=LK_ROW, **NEW) == "kv_append_lk:wg=256:lds=0;fwd_lk:wg=256:lds=36864"
    assert code(L, args(L, 1, 64, kv_dtype=1)) == EINVAL


def test_lk_row_refusals(L):
    ok = dict(lk_row=LK_ROW)
    assert code(L, args(L, 1, 17, **ok)) == 0
    assert code(L, args(L, 2, 17, **ok)) == EINVAL                                         # Lq != 1
    assert code(L, args(L, 1, 17, drop_p=0.1, **ok)) == EINVAL                             # dropout
    assert code(L, args(L, 1, 17, kv_index=KV_INDEX, **ok)) == EINVAL                      # the table without its offsets
    assert code(L, args(L, 1, 17, kv_index=KV_INDEX, kv_index_off=KV_OFF, **ok)) == 0
    bw = args(L, 1, 17, p=0x50000, d_o=0x60000, dq=0x70000, d_k=0x80000, dv=0x90000, **ok)
    assert code(L, bw, bwd=True) == EINVAL                                                 # the backward
    bw.lk_row = None
    assert code(L, bw, bwd=True) == 0
    assert code(L, args(L, 1, 17, dk=8, **ok)) == 0 and code(L, args(L, 3, 17, dk=8, **ok)) == EINVAL
    # a call only the bf16-operand kernels take (precision 1, more than 48 fp32 keys in the regular layout) has no lk_row instance
    assert code(L, args(L, 1, 64, precision=1)) == 0 and code(L, args(L, 1, 64, precision=1, **ok)) == EINVAL
    assert code(L, args(L, 1, 64, precision=1, kv_group_stride=64, **ok)) == 0


# ------------------------------------------------------------------------------------------------ workspace and options
def _model(precision=0, **over):
    import sparse_image_captioning_amd as P
    from sparse_image_captioning_amd.utils.config import Config
    return P.get_model("relation_transformer")(Config(**dict(C.TINY_CFG, **over)), precision=precision)


@pytest.mark.parametrize("precision", [0, 1])
def test_workspace_bytes_with_the_joint_flag(L, precision):
    lib = L.lib()
    m = _model(precision)

    def nbytes(**kw):
        o = L.DecodeOpts()
        o.beam_size, o.temperature, o.diversity_lambda = 6, 1.0, 0.5
        for k, v in kw.items():
            setattr(o, k, v)
        return lib.ortk_decode_workspace_bytes(Ct.byref(m._ccfg), 4, 9, Ct.byref(o))

    JOINT = L.DEC_GROUPS_JOINT
    assert JOINT >= 1 << 16
    for b, G in ((6, 3), (32, 4)):
        staggered = nbytes(beam_size=b, group_size=G, exec_flags=L.DEC_UNFUSED)
        joint = nbytes(beam_size=b, group_size=G, exec_flags=L.DEC_UNFUSED | JOINT)
        assert staggered > 0 and joint > staggered, (b, G, staggered, joint)
        assert nbytes(beam_size=b, group_size=G, exec_flags=JOINT) == joint == nbytes(beam_size=b, group_size=G, exec_flags=JOINT | L.DEC_SPLIT_SMALL)
    for kw in ({"group_size": 1}, {"group_size": 0}, {"group_size": 3, "train": 1}, {"group_size": 3, "beam_size": 0, "num_random_sample": 3},
               {"group_size": 1, "beam_size": 0, "num_random_sample": 3}, {"group_size": 1, "beam_size": 0, "num_random_sample": 3, "train": 1},
               {"group_size": 3, "exec_flags": L.DEC_STACK}, {"group_size": 3, "exec_flags": L.DEC_SPARSE_STREAM},
               {"group_size": 3, "exec_flags": L.DEC_STACK | L.DEC_STACK_SPLIT}, {"group_size": 3, "exec_flags": L.DEC_STACK | L.DEC_STACK_RB20},
               {"group_size": 3, "exec_flags": L.DEC_SPARSE_STREAM | L.DEC_SPARSE_GATHER}, {"group_size": 3, "exec_flags": L.DEC_STACK | L.DEC_STACK_FP8}):
        kw = dict(kw, exec_flags=kw.get("exec_flags", 0) | JOINT)
        assert nbytes(**kw) == 0, kw
    # the same options without the flag keep their answers
    assert nbytes(group_size=1) > 0 and nbytes(group_size=1, beam_size=0, num_random_sample=3) > 0


def test_decode_opts_unfused_joint(L):
    m = _model()
    o, K, ex = m._decode_opts({"beam_size": 6, "group_size": 3, "executor": "unfused_joint", "seed": 1})
    assert (o.group_size, K, ex) == (3, 6, "unfused_joint")
    assert o.exec_flags == L.DEC_UNFUSED | L.DEC_GROUPS_JOINT
    # the other executors keep their flags: never the joint bit
    for ex_ in ("auto", "unfused"):
        assert not (m._decode_opts({"beam_size": 6, "group_size": 3, "executor": ex_, "seed": 1})[0].exec_flags & L.DEC_GROUPS_JOINT)
    assert not (m._decode_opts({"beam_size": 6, "group_size": 3, "seed": 1})[0].exec_flags & L.DEC_GROUPS_JOINT)
    for opt, why in (({"beam_size": 6}, "needs group_size > 1"),
                     ({"beam_size": 6, "group_size": 1}, "needs group_size > 1"),
                     ({"beam_size": 0, "num_random_sample": 3}, "does not serve num_random_sample > 0"),
                     ({"beam_size": 0, "num_random_sample": 3, "group_size": 3}, "does not serve num_random_sample > 0"),
                     ({"beam_size": 6, "group_size": 3, "train_mode": True, "drop_seed": 1}, "does not serve train_mode"),
                     ({"beam_size": 6, "group_size": 4}, "not a multiple of group_size=4")):
        with pytest.raises(ValueError, match=why):
            m._decode_opts(dict(opt, executor="unfused_joint", seed=1))
        assert not m.decode_supported(4, 9, dict(opt, executor="unfused_joint")), opt
    # the refusal of the stack executors for groups keeps its wording
    with pytest.raises(ValueError, match='executor="stack" does not serve group_size=2: diverse beam groups decode at different positions, '
                                         'the stack kernels take one position per launch; use "auto" or "unfused"'):
        m._decode_opts({"beam_size": 4, "group_size": 2, "executor": "stack", "seed": 1})
    assert m.decode_supported(4, 9, {"beam_size": 6, "group_size": 3, "executor": "unfused_joint"})
    assert m.decode_supported(4, 9, {"beam_size": 20, "group_size": 20, "executor": "unfused_joint"})      # more groups than positions


# ------------------------------------------------------------------------------------------------ the edge cases' inputs
@pytest.mark.parametrize("case", list(J.EDGE_CASES))
def test_edge_case_seeds_leave_enough_images_with_a_margin(case):
    """The restatement alone: at least half of the images of every edge-schedule case have min_gap >= GAP on the recorded seed."""
    b, G, opts, seed, need = J.EDGE_CASES[case]
    assert need * 2 >= D.N_IMG
    gap = J.restated(case)[1][3]
    assert int((gap >= D.GAP).sum()) >= need, (case, gap.tolist())
    if case == "b20_g20":
        assert G > C.TINY_CFG["max_seq_length"]                     # groups finish before others start
