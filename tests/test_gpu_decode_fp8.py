"""The FP8 weight stream of the decoder stack kernel (`executor="stack_fp8"`, ORTK_DEC_STACK_FP8) and its quantiser (ortk_fp8_rows).

An e4m3 value times a power of two is a bf16 value, so the kernel that dequantises in registers feeds its MFMAs exactly what the bf16
stream would on the dequantised weights W': every executor comparison below is `torch.equal`, no tolerance.  The refusal / size checks
are host-side arithmetic of the library and need no GPU."""
import ctypes as C

import pytest
import torch

import common as Cm
import fp8_ref as R
import helpers as H

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import sparse_image_captioning_amd as pkg
    return pkg


def _model(P, cfg, state=None, precision=1, **over):
    from sparse_image_captioning_amd.utils.config import Config
    m = P.get_model("relation_transformer")(Config(**dict(cfg, **over)), precision=precision)
    if state is not None:
        missing, unexpected = m.load_state_dict(state, strict=False)
        assert not unexpected and all(k.endswith(".pe") for k in missing), (missing, unexpected)
    return m


def _cuda(b):
    return {k: v.cuda() for k, v in b.items()}


@pytest.fixture(scope="module")
def margin_state():
    """Full-size weights with real decision margins (generator x 3, EOS bias: tests/test_gpu_model.py::margin_state)."""
    return H.torch_state(H.dense_param_shapes(Cm.FULL_CFG), Cm.G2_SEED, Cm.G1_GEN_SCALE, Cm.G1_EOS_BIAS)


@pytest.fixture(scope="module")
def pair(P, margin_state):
    """(m, m2): the model, and the same state with its own dequantised decoder weights W' loaded over it."""
    P._lib.require_gpu()
    m = _model(P, Cm.FULL_CFG, margin_state).cuda().eval()
    m2 = _model(P, Cm.FULL_CFG, margin_state).cuda().eval()
    _load_dequantized(m, m2)
    return m, m2


def _load_dequantized(m, m2):
    deq = m.fp8_dequantized_decoder_state()
    missing, unexpected = m2.load_state_dict(dict(m.state_dict(), **deq), strict=True)
    assert not missing and not unexpected
    return deq


@pytest.fixture(scope="module")
def batches():
    """70 images x 12-36 regions and 37 images x 33-100 regions: partial last row blocks, images straddling blocks."""
    return {n_reg: _cuda(H.torch_batch(Cm.make_inputs(seed=41, n_img=n_img, n_reg=n_reg, feat=2048, vocab=10001, spi=1, ragged=True)))
            for n_reg, n_img in ((36, 70), (100, 37))}


def _decode(m, b, opt, executor):
    with torch.no_grad():
        seq, lp = m(att_feats=b["att_feats"], boxes=b["boxes"], att_masks=b["att_masks"], opt=dict(opt, executor=executor), mode="sample")
    return seq.clone(), lp.clone(), m._last_decode[2].clone()


def _assert_same(a, b, what):
    for x, y, name in zip(a, b, ("tokens", "log-probs", "scores")):
        assert torch.equal(x, y), (what, name, (x != y).float().mean().item())


# ------------------------------------------------------------------------------------------------ 1. the quantiser
@gpu
def test_fp8_rows_equals_cpu_torch(P):
    """Bytes, scales and dequantised image of ortk_fp8_rows against CPU torch (exact power-of-two scaling, RNE `.to(float8_e4m3fn)`)
    on 67 rows x 1 024 columns with ld = 1 100: normal rows from 1e-6 to 1e4, an all-zero group, a group with one non-zero, -0.0, amax
    exactly 448 x 2^k and one bf16 ulp above, exact ties of both parities, e4m3's subnormal range and values below half its smallest
    subnormal.  Equality, and the same bytes from a second run."""
    L = P._lib
    L.require_gpu()
    w16, where = R.edge_weights()
    q_ref, sc_ref, deq_ref = R.fp8_rows_ref(w16)
    for name, at in where.items():                         # the classes are there, and the reference treats them as the contract says
        if name.startswith("amax_"):
            assert float(sc_ref[at[0], at[1]]) == 2.0 ** at[2], name
    assert float(sc_ref[where["all_zero"]]) == 1.0 and int(q_ref[40, :512].max()) == 0
    assert int((q_ref[41, 512:] & 0x7F != 0).sum()) == 1
    assert int((q_ref[42, :512] == 0x80).sum()) >= 20      # -0.0 keeps its sign
    rows, n_cols, ld = 67, 1024, 1100
    buf = torch.full((rows, ld), float("nan"), dtype=torch.bfloat16)
    buf[:, :n_cols] = w16
    buf = buf.cuda()
    outs = []
    for _ in range(2):
        q = torch.full((rows, n_cols), 0xAA, dtype=torch.uint8, device="cuda")
        sc = torch.zeros(rows, n_cols // 512, device="cuda")
        deq = torch.full((rows, n_cols), float("nan"), device="cuda")
        L.check(L.lib().ortk_fp8_rows(L.ptr(buf), ld, rows, n_cols, L.ptr(q), n_cols, L.ptr(sc), L.ptr(deq), n_cols, L.stream_ptr()), "ortk_fp8_rows")
        outs.append((q.cpu(), sc.cpu(), deq.cpu()))
    q, sc, deq = outs[0]
    bad = (q != q_ref).nonzero()
    assert bad.numel() == 0, [(int(r), int(c), float(w16[r, c]), int(q[r, c]), int(q_ref[r, c])) for r, c in bad[:8]]
    assert torch.equal(sc, sc_ref)
    assert torch.equal(deq, deq_ref) and torch.equal(deq.view(torch.int32) >> 31, deq_ref.view(torch.int32) >> 31)      # signs of zeros too
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    # without the dequantised image; and the argument checks
    q2 = torch.empty_like(q, device="cuda")
    sc2 = torch.empty_like(sc, device="cuda")
    L.check(L.lib().ortk_fp8_rows(L.ptr(buf), ld, rows, n_cols, L.ptr(q2), n_cols, L.ptr(sc2), None, 0, L.stream_ptr()), "ortk_fp8_rows")
    assert torch.equal(q2.cpu(), q_ref) and torch.equal(sc2.cpu(), sc_ref)
    assert L.lib().ortk_fp8_rows(L.ptr(buf), ld, rows, 1000, L.ptr(q2), n_cols, L.ptr(sc2), None, 0, L.stream_ptr()) == -1
    assert L.lib().ortk_fp8_rows(L.ptr(buf), 1022, rows, n_cols, L.ptr(q2), n_cols, L.ptr(sc2), None, 0, L.stream_ptr()) == -1


# ------------------------------------------------------------------------------------------------ 2. the executor
OPTS = [{"beam_size": 1}, {"beam_size": 5}, {"beam_size": 3, "decoding_constraint": 1}, {"num_random_sample": 3, "beam_size": 0, "seed": 7}]


@gpu
@pytest.mark.parametrize("n_reg", [36, 100])
@pytest.mark.parametrize("opt", OPTS, ids=["greedy", "beam5", "beam3_constraint", "sample3"])
def test_stack_fp8_is_bit_identical_to_stack_on_dequantized_weights(pair, batches, n_reg, opt):
    """`stack_fp8` on W against `stack` on W' = fp8_dequantized_decoder_state(): tokens, log-probs and beam scores equal bit for bit."""
    m, m2 = pair
    _assert_same(_decode(m, batches[n_reg], opt, "stack_fp8"), _decode(m2, batches[n_reg], opt, "stack"), (n_reg, opt))


@gpu
def test_stack_fp8_is_bit_identical_on_long_captions(P, batches):
    """The same comparison on weights whose captions run long: under `margin_state`'s EOS bias the best caption of these random-weight
    models ends at once, so the rows of a greedy decode stop mattering after the first position.  Generator x 3 WITHOUT the EOS bias
    gives 16-token captions, different for every image: every position of every row is compared."""
    P._lib.require_gpu()
    state = H.torch_state(H.dense_param_shapes(Cm.FULL_CFG), Cm.G2_SEED, Cm.G1_GEN_SCALE, 0.0)
    m = _model(P, Cm.FULL_CFG, state).cuda().eval()
    m2 = _model(P, Cm.FULL_CFG, state).cuda().eval()
    _load_dequantized(m, m2)
    for n_reg in (36, 100):
        for opt in OPTS:
            got = _decode(m, batches[n_reg], opt, "stack_fp8")
            _assert_same(got, _decode(m2, batches[n_reg], opt, "stack"), (n_reg, opt))
            if opt == {"beam_size": 1}:
                assert (got[0] != 0).sum(-1).float().mean().item() > 8 and len({tuple(r.tolist()) for r in got[0][:, 0]}) > got[0].size(0) // 2


@gpu
def test_stack_fp8_quantizes_something(pair, batches):
    """W' is not W (the comparison above is not vacuous), only the six decoder weight families are listed, every entry is within the
    rounding error of the format of the bf16 weight, and the quantised decode differs from the unquantised one."""
    m, m2 = pair
    deq = m.fp8_dequantized_decoder_state()
    sd = m.state_dict()
    assert len(deq) == 6 * 8 and all(".decoder.layers." in k and k.endswith(".weight") and ".src_attn.linears.1." not in k
                                      and ".src_attn.linears.2." not in k for k in deq)
    for k, v in deq.items():
        w = sd[k].bfloat16().float()
        assert v.shape == w.shape and not torch.equal(v, w)
        # round to nearest of a 3-bit mantissa: within 2^-4 relative of a value in e4m3's normal range; below it within half a subnormal
        # step, 2^-10 x scale, and the scale is below amax / 224 (amax / scale lies in (224, 448]): < amax x 2^-17
        amax = w.view(w.size(0), -1, 512).abs().amax(-1, keepdim=True)
        err = (v - w).view(w.size(0), -1, 512).abs()
        assert bool((err <= torch.maximum(w.view_as(err).abs() * 2.0 ** -4, amax * 2.0 ** -17)).all()), k
    _, l8, _ = _decode(m, batches[36], {"beam_size": 1}, "stack_fp8")
    _, l16, _ = _decode(m, batches[36], {"beam_size": 1}, "stack")
    assert not torch.equal(l8, l16)


@gpu
def test_stack_fp8_shared_layers_and_long_captions(P, margin_state):
    """ACORT-style decoder (layers shared in pairs, d_ff 1 024: two hidden chunks, 26-token captions) and 40-token captions (more cached
    keys than one self-attention batch, `seq_length` 40), as test_decoder_stack_kernel_shared_layers_and_long_captions has."""
    P._lib.require_gpu()
    b = _cuda(H.torch_batch(Cm.make_inputs(seed=43, n_img=33, n_reg=36, feat=2048, vocab=10001, spi=1, ragged=True)))
    cfg = dict(Cm.FULL_CFG, max_seq_length=26, dim_feedforward=1024, share_layer_decoder=(0, 0, 1, 1, 2, 2))
    torch.manual_seed(3)
    m = _model(P, cfg).cuda().eval()
    m2 = _model(P, cfg).cuda().eval()
    deq = _load_dequantized(m, m2)
    assert len(deq) == 6 * 8 and deq["model.decoder.layers.1.feed_forward.w_2.weight"] is deq["model.decoder.layers.0.feed_forward.w_2.weight"]
    _assert_same(_decode(m, b, {"beam_size": 5}, "stack_fp8"), _decode(m2, b, {"beam_size": 5}, "stack"), "share_layer")
    m = _model(P, Cm.FULL_CFG, margin_state, max_seq_length=40).cuda().eval()
    m2 = _model(P, Cm.FULL_CFG, margin_state, max_seq_length=40).cuda().eval()
    _load_dequantized(m, m2)
    for opt in ({"beam_size": 5}, {"num_random_sample": 3, "beam_size": 0, "seed": 11}):
        _assert_same(_decode(m, b, opt, "stack_fp8"), _decode(m2, b, opt, "stack"), ("seq_length 40", opt))


# ------------------------------------------------------------------------------------------------ 3. determinism and state
@gpu
def test_stack_fp8_is_deterministic_and_follows_the_weights(P, margin_state, batches):
    """Two decodes give equal bits; after a decoder weight changes in place the next decode equals `stack` on the NEW W': the stream is
    rebuilt from the weights of every call."""
    P._lib.require_gpu()
    m = _model(P, Cm.FULL_CFG, margin_state).cuda().eval()
    m2 = _model(P, Cm.FULL_CFG, margin_state).cuda().eval()
    b, opt = batches[36], {"beam_size": 5}
    first = _decode(m, b, opt, "stack_fp8")
    _assert_same(first, _decode(m, b, opt, "stack_fp8"), "rerun")
    with torch.no_grad():
        w = dict(m.named_parameters())["model.decoder.layers.2.feed_forward.w_1.weight"]
        w[5:900:3] *= -1.5
        dict(m.named_parameters())["model.decoder.layers.0.self_attn.linears.1.weight"][:, 7] = 0.3
    _load_dequantized(m, m2)
    second = _decode(m, b, opt, "stack_fp8")
    assert not torch.equal(first[1], second[1])
    _assert_same(second, _decode(m2, b, opt, "stack"), "after the in-place change")


# ------------------------------------------------------------------------------------------------ 4. refusals and sizes (host side)
def _opts(L, flags, **kw):
    o = L.DecodeOpts()
    o.beam_size, o.temperature, o.exec_flags = 5, 1.0, flags
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_stack_fp8_refusals_and_workspace_sizes(P):
    L = P._lib
    lib = L.lib()
    assert L.DEC_STACK_FP8 == 128
    m = _model(P, Cm.FULL_CFG)
    m32 = _model(P, Cm.FULL_CFG, precision=0)
    nbytes = lambda mod, o, B=70, S=36: lib.ortk_decode_workspace_bytes(C.byref(mod._ccfg), B, S, C.byref(o))
    fp8 = L.DEC_STACK_FP8
    # served: alone (it implies ORTK_DEC_STACK) and with ORTK_DEC_STACK, at any row count
    for B in (1, 70, 1024):
        assert nbytes(m, _opts(L, fp8), B) == nbytes(m, _opts(L, fp8 | L.DEC_STACK), B) > 0
    # refused: every listed combination returns 0 bytes
    for other in (L.DEC_SPARSE_STREAM, L.DEC_SPARSE_STREAM | L.DEC_SPARSE_GATHER, L.DEC_SPARSE_GATHER, L.DEC_STACK_SPLIT, L.DEC_SPLIT_SMALL,
                  L.DEC_STACK_RB20, L.DEC_UNFUSED):
        assert nbytes(m, _opts(L, fp8 | L.DEC_STACK | other)) == 0, other
        assert nbytes(m, _opts(L, fp8 | other)) == 0, other
    assert nbytes(m32, _opts(L, fp8)) == 0 and nbytes(m32, _opts(L, fp8 | L.DEC_STACK)) == 0                 # fp32 precision
    plan = L.EllPlanStruct()
    assert nbytes(m, _opts(L, fp8, sparse=C.pointer(plan))) == 0                                              # a sparse plan
    samp = dict(beam_size=0, num_random_sample=5)
    assert nbytes(m, _opts(L, fp8, **samp)) > 0 and nbytes(m, _opts(L, fp8, train=1, drop_seed=3, **samp)) == 0      # train
    # the stream is smaller than the bf16 one by the difference of the packed sizes: 14 units of 512 x 512 weights per layer at 1 byte
    # instead of 2, plus 4 bytes of scale per weight row and unit (and the rings' read-ahead: 8 k-steps of 2 KB against 4 of 4 KB)
    n_units = 6 * (6 + 2 * (2048 // 512))
    packed16 = n_units * 512 * 512 * 2 + 4 * 4096
    packed8 = n_units * 512 * 512 + 8 * 2048 + (n_units * 512 + 64) * 4
    for B in (70, 1024):
        d = nbytes(m, _opts(L, L.DEC_STACK), B) - nbytes(m, _opts(L, fp8), B)
        assert d >= packed16 - packed8 - 512 > 20e6, (B, d)


def test_stack_fp8_model_refusals_raise_value_error(P):
    m32 = _model(P, Cm.FULL_CFG, precision=0)
    with pytest.raises(ValueError, match="mixed precision"):
        m32._decode_opts({"beam_size": 5, "executor": "stack_fp8"})
    m = _model(P, Cm.FULL_CFG)
    o, K, ex = m._decode_opts({"beam_size": 5, "executor": "stack_fp8", "seed": 0})
    assert ex == "stack_fp8" and o.exec_flags == P._lib.DEC_STACK | P._lib.DEC_STACK_FP8
    assert m.decode_supported(70, 36, {"beam_size": 5, "executor": "stack_fp8"})
    with pytest.raises(ValueError, match="train-mode"):
        m._decode_opts({"beam_size": 0, "num_random_sample": 5, "executor": "stack_fp8", "train_mode": True, "drop_seed": 3})
    m._sparse_min = 0.9                     # what enable_sparse_kernels() records (its plans need a device)
    with pytest.raises(ValueError, match="sparse plan"):
        m._decode_opts({"beam_size": 5, "executor": "stack_fp8"})
    kv = _model(P, Cm.FULL_CFG, share_att_decoder="kv")
    with pytest.raises(ValueError, match="share_att_decoder"):
        kv._decode_opts({"beam_size": 5, "executor": "stack_fp8"})
    # never chosen automatically
    for opt in ({"beam_size": 5}, {"beam_size": 5, "executor": "stack"}, {"beam_size": 5, "executor": "auto"}):
        assert not (_model(P, Cm.FULL_CFG)._decode_opts(dict(opt, seed=0))[0].exec_flags & P._lib.DEC_STACK_FP8)
