"""Exact GEMM tests, CPU side: the operand classes of tests/gemm_exact.py really are exact (bounds, bf16 parts, order independence) for
every case of the table the GPU runs, and ortk_gemm_plan — which launches nothing and needs no device — names the kernel each case is
meant for."""
import ctypes as C

import pytest
import torch

import gemm_exact as X


@pytest.fixture(scope="module")
def L():
    import sparse_image_captioning_amd as P
    P._lib.lib()
    return P._lib


def _fake_args(L, c):
    return X.fake_args(c, L.GemmArgs())


def _plan(L, c):
    prev = L.set_tuning(**c.tuning)
    try:
        return L.gemm_plan(_fake_args(L, c))
    finally:
        L.set_tuning(**prev)


def test_plan_query_answers_without_a_device(L):
    lib = L.lib()
    c = next(k for k in X.CASES if k.name == "nsplit_lean1")
    a = _fake_args(L, c)
    assert L.gemm_plan(a) == ["bf16_dma256<1>", "bf16_glds<0,1>"]
    prev = L.set_tuning(gemm_epilogue=2)          # (read as the call reads it: never split the column count)
    try:
        assert L.gemm_plan(a) == ["bf16_glds<0,1>"]
    finally:
        L.set_tuning(**prev)
    assert L.gemm_plan(a) == ["bf16_dma256<1>", "bf16_glds<0,1>"]
    # the launches around the plan, in stream order
    assert _plan(L, next(k for k in X.CASES if k.name == "f32_tt_colsum_TxW3")) == ["colsum", "f32<1,1>"]
    assert _plan(L, next(k for k in X.CASES if k.name == "ln_fwd_separate")) == ["bf16<0,0,f32,f32,0>", "layernorm_fwd"]
    assert _plan(L, next(k for k in X.CASES if k.name == "ln_fwd_fused")) == ["bf16_row512"]
    # an empty product launches nothing; a buffer that is too short is refused, never overrun
    z = L.GemmArgs.from_buffer_copy(a); z.M = 0
    assert L.gemm_plan(z) == []
    buf = C.create_string_buffer(b"#" * 40, 40)
    assert lib.ortk_gemm_plan(C.byref(a), buf, 8) == -2 and buf.raw == b"#" * 40
    assert lib.ortk_gemm_plan(C.byref(a), buf, 30) == 0 and buf.value == b"bf16_dma256<1>;bf16_glds<0,1>"
    assert lib.ortk_gemm_plan(C.byref(a), None, 30) == -1
    # what ortk_gemm refuses, refused with its code
    bad = []
    for edit in (dict(A=0), dict(K=-1), dict(a_dtype=2), dict(transA=1, transB=0), dict(accumulate=1, c_dtype=1), dict(colsum=0x40, transA=0),
                 dict(precision=0), dict(ln_mode=3), dict(ln_mode=1, ln_a=0x40, ln_stats=0x80), dict(tile_samp=0x40), dict(tile_stats=0x40, stat_ncols=0)):
        b = L.GemmArgs.from_buffer_copy(a)
        for k, v in edit.items():
            setattr(b, k, v)
        bad.append(lib.ortk_gemm_plan(C.byref(b), buf, 40))
    assert bad == [-1] * len(bad)
    assert lib.ortk_gemm_plan(None, buf, 40) == -1


def test_every_case_plans_the_kernel_it_is_meant_for_and_the_table_covers_the_file(L):
    seen = set()
    for c in X.CASES:
        got = _plan(L, c)
        assert got == c.plan, (c.name, got)
        seen.update(got)
    assert sorted(seen) == X.INSTANCES
    assert not seen & set(X.EXCLUDED)


def test_the_instance_list_matches_the_kernels_of_the_source():
    """Every name ortk_gemm.hip can report is either in the list the table must cover or excluded with a reason."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sparse-image-captioning_amd", "csrc", "ortk_gemm.hip")).read()
    # ORTK_INST(family, args) / ORTK_ADD_F32X3 form a kernel instance and its name from one text; ORTK_INST0 a kernel that is no
    # template; ORTK_ROWLN(MT) a LayerNorm-backward panel; ORTK_PICK16(TA, TB, FAST) the four operand-type instances of gemm_bf16_kernel
    names = {f"{f}<{a}>" for f, a in re.findall(r"\bORTK_(?:INST|ADD_F32X3)\((\w+), ([-0-9,]+)\)", src)}
    names |= set(re.findall(r"\bORTK_INST0\((\w+)\)", src)) - {"family"}
    names |= {f"bf16_rowln_bwd<{mt}>" for mt in re.findall(r"\bORTK_ROWLN\((\d)\)", src)}
    for ta, tb, fast in re.findall(r"\bORTK_PICK16\((\d), (\d), (\d)\)", src):
        names |= {f"bf16<{ta},{tb},{a},{b},{fast}>" for a in ("f32", "bf16") for b in ("f32", "bf16")}
    names |= set(re.findall(r'"(colsum|layernorm_[a-z_]+)"', src))       # what ortk_gemm launches around the plan
    assert not re.search(r'Inst\{[^}#]*"', src)                  # (outside those macros, no name written out beside an instance)
    assert names == set(X.INSTANCES) | set(X.EXCLUDED), sorted(names ^ (set(X.INSTANCES) | set(X.EXCLUDED)))


def test_operand_classes_need_the_parts_they_are_named_for():
    for cls, want in X.PARTS.items():
        x = X.GEN[cls](300, 96, 7)
        assert torch.equal(x, x.round()) and (x == 0).any()
        parts, rest = X.bf16_parts(x)
        assert torch.equal(sum(p.double() for p in parts), x) and not rest.any(), cls       # the split is exact
        need = X.parts_needed(x)[x != 0]
        assert int(need.max()) == want, cls
        if want > 1:
            assert (need == want).float().mean().item() >= 0.25, cls
        if cls in ("T", "W2s"):
            assert int((x != 0).sum(1).max()) <= 15
    # 17-bit integers still split into two round-to-nearest parts
    assert int(X.parts_needed(torch.arange(2 ** 16, 2 ** 17, dtype=torch.float64)).max()) == 2


@pytest.mark.parametrize("c", X.CASES, ids=lambda c: c.name)
def test_case_is_exact_in_fp32(c):
    """Bounds in float64, the bf16 parts of both operands, and an fp32 accumulation in random k orders against the float64 product.
    (The order check walks at most 512 rows of a case — its first and last 256 — where the whole product is over 2^26 terms.)"""
    o = X.operands(c)
    for k, v in X.bound(c, o).items():
        assert v < X.LIM, (k, v)
    for k, cls in zip(("A", "B"), c.cls):
        x = o[k]
        parts, rest = X.bf16_parts(x)
        assert torch.equal(sum(p.double() for p in parts), x) and not rest.any()
        nz = X.parts_needed(x)[x != 0]
        if nz.numel():
            assert int(nz.max()) <= X.PARTS[cls]
            if X.PARTS[cls] > 1:
                assert (nz == X.PARTS[cls]).float().mean().item() >= 0.25
        if c.prec:
            assert X.PARTS[cls] == 1      # the bf16 MFMA path rounds its operands to one part
        assert (x == 0).any() or x.numel() < 64
    if not c.prec:
        assert c.cls in X.PAIRINGS        # every product of two parts is among the six the split kernels keep
    A, B = o["A"], o["B"]
    if c.M * c.N * c.K > 2 ** 26:
        A = torch.cat([A[:256], A[-256:]])
    ref = A @ B.t()
    g = torch.Generator().manual_seed(c.seed)
    A32, B32 = A.float(), B.float()
    for _ in range(3):
        acc = torch.zeros(A.shape[0], c.N)
        for k in torch.randperm(c.K, generator=g).tolist():
            acc += A32[:, k, None] * B32[None, :, k]
        assert torch.equal(acc.double(), ref)
    # the whole epilogue, in fp32, equals its float64 reference (a fixed keep pattern stands in for the replayed draws)
    keep = ((torch.arange(c.M)[:, None] + torch.arange(c.N)[None, :]) % 2 * 2).double() if c.drop else None
    want, _ = X.expected(c, o, keep)
    assert torch.equal(want.float().double(), want)
