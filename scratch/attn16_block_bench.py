"""The two block shapes of the training step's bf16 attention alone (H = 8, dk = 64, bf16 Q|K|V packed, bf16 outputs, probability
dropout 0.1), forward and backward, at ortk_tuning.attn16_block = 0 (a wave per query tile, every operand an LDS image) and 1
(operands from global memory / one shared image: more workgroups per compute unit):
  enc     256 x 8 x 36 x 36, geometry bias, dscore
  cross   256 x 8 x 85 x 36, the padded rectangle
  crossv  the same on the valid-position layout (q_off stride 5, drop_rows, caption lengths 9..17)
Interleaved, three rounds of 50 launches each; also checks that the outputs of both settings are bit-identical.
`sweep` as the first argument times the encoder shape at 96 .. 384 images instead (rounds of workgroups: profiles/attn16_block.txt
§1).  A library without the switch (the parent's) runs its only mapping."""
import ctypes as C, hashlib, os, socket, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sparse_image_captioning_amd as P
L = P._lib
L.require_gpu()
print("box", socket.gethostname(), " lib md5", hashlib.md5(open(L.LIB_PATH, "rb").read()).hexdigest(), flush=True)
H, dk, S, T, spi = 8, 64, 36, 17, 5
d = H * dk
HAS = "attn16_block" in L.set_tuning()
SETTINGS = (0, 1) if HAS else (0,)


def setting(v):
    if HAS: L.set_tuning(attn16_block=v)


def build(kind, nimg):
    """The argument block of one shape and the tensors it points to."""
    g = torch.Generator().manual_seed(3)
    Lq = S if kind == "enc" else spi * T
    if kind == "crossv":
        lengths = torch.randint(9, T + 1, (nimg * spi,), generator=torch.Generator().manual_seed(11)).tolist()
    else:
        lengths = None
    off = [0]
    for n in lengths or []: off.append(off[-1] + n)
    Mq = off[-1] if lengths else nimg * Lq
    Mk = nimg * S
    a = L.AttnArgs()
    a.precision, a.qkv_dtype, a.o_dtype, a.dqkv_dtype = 1, 1, 1, 1
    hold = []
    if kind == "enc":
        qkv = torch.randn(Mq, 3 * d, generator=g).bfloat16().cuda(); dqkv = torch.empty(Mq, 3 * d, device="cuda", dtype=torch.bfloat16)
        a.q, a.k, a.v = qkv.data_ptr(), qkv.data_ptr() + 2 * d, qkv.data_ptr() + 4 * d
        a.ldq = a.ldk = a.ldv = 3 * d
        a.dq, a.d_k, a.dv = dqkv.data_ptr(), dqkv.data_ptr() + 2 * d, dqkv.data_ptr() + 4 * d
        a.lddq = a.lddk = a.lddv = 3 * d
        bias = torch.randn(nimg, H, S, S, generator=g).cuda(); ds = torch.empty(nimg, H, S, S, device="cuda")
        a.bias, a.dscore = bias.data_ptr(), ds.data_ptr()
        outs = [dqkv, ds]; hold += [qkv, bias]
    else:
        q = torch.randn(Mq, d, generator=g).bfloat16().cuda(); kv = torch.randn(Mk, 2 * d, generator=g).bfloat16().cuda()
        dq = torch.empty(Mq, d, device="cuda", dtype=torch.bfloat16); dkv = torch.empty(Mk, 2 * d, device="cuda", dtype=torch.bfloat16)
        a.q, a.k, a.v = q.data_ptr(), kv.data_ptr(), kv.data_ptr() + 2 * d
        a.ldq, a.ldk, a.ldv = d, 2 * d, 2 * d
        a.dq, a.d_k, a.dv = dq.data_ptr(), dkv.data_ptr(), dkv.data_ptr() + 2 * d
        a.lddq, a.lddk, a.lddv = d, 2 * d, 2 * d
        outs = [dq, dkv]; hold += [q, kv]
        if lengths:
            qo = torch.tensor(off, dtype=torch.int32).cuda()
            rp = torch.tensor([c * T + t for c, n in enumerate(lengths) for t in range(n)], dtype=torch.int32).cuda()
            a.q_off, a.q_off_stride, a.drop_rows = qo.data_ptr(), spi, rp.data_ptr()
            hold += [qo, rp]
    do = torch.randn(Mq, d, generator=g).bfloat16().cuda(); o = torch.empty(Mq, d, device="cuda", dtype=torch.bfloat16)
    p = torch.zeros(nimg, H, Lq, S, device="cuda"); km = torch.ones(Mk, device="cuda")
    a.o, a.p, a.kmask, a.ldo, a.d_o, a.lddo = o.data_ptr(), p.data_ptr(), km.data_ptr(), d, do.data_ptr(), d
    a.nkv, a.H, a.Lq, a.Lk, a.dk, a.drop_p, a.drop_seed = nimg, H, Lq, S, dk, 0.1, 5
    return a, [o, p] + outs, hold + [do, km]


def md5s(ts):
    torch.cuda.synchronize()
    return [hashlib.md5(t.cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().tobytes()).hexdigest() for t in ts]


def timed(fn, a, n=50):
    for _ in range(3): L.check(fn(C.byref(a), L.stream_ptr()), "attention")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn(C.byref(a), L.stream_ptr())
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n


def case(kind, nimg, rounds=3):
    a, outs, hold = build(kind, nimg)
    fns = (("fwd", L.lib().ortk_attention_fwd), ("bwd", L.lib().ortk_attention_bwd))
    res, sums = {}, {}
    for rep in range(rounds):
        for sw in SETTINGS:
            setting(sw)
            for fname, fn in fns: res.setdefault((sw, fname), []).append(timed(fn, a))
            sums[sw] = md5s(outs)
    setting(1)
    for sw in SETTINGS:
        print(f"{kind:6s} {nimg:4d} images  attn16_block={sw}: fwd us {' '.join(f'{x:6.1f}' for x in res[(sw, 'fwd')])}   bwd us {' '.join(f'{x:6.1f}' for x in res[(sw, 'bwd')])}"
              f"   outputs {'== attn16_block=0' if sums[sw] == sums[0] else 'DIFFER'}", flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "sweep":
    for n in (96, 192, 200, 256, 384): case("enc", n)
else:
    for kind in ("enc", "cross", "crossv"): case(kind, 256)
