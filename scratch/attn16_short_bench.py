"""The decoder self-attention of the bench shape alone (1 280 captions x 8 heads x 17 x 17, causal, bf16 Q|K|V packed with a
1 536-element pitch, bf16 outputs, probability dropout 0.1), forward and backward, at ortk_tuning.attn16_short = 0 (block
kernels), 4 and 8 (short kernels, that many waves per workgroup): the padded rectangle and the valid-position layout with caption
lengths 9..17.  Interleaved, three rounds of 50 launches each; also checks that the outputs of every setting are bit-identical."""
import ctypes as C, hashlib, os, socket, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sparse_image_captioning_amd as P
L = P._lib
L.require_gpu()
print("box", socket.gethostname(), " lib md5", hashlib.md5(open(L.LIB_PATH, "rb").read()).hexdigest(), flush=True)
ncap, H, T, dk = 1280, 8, 17, 64
d = H * dk


def case(name, lengths):
    off = [0]
    for n in lengths: off.append(off[-1] + n)
    M = off[-1]
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(M, 3 * d, generator=g).bfloat16().cuda()
    do = torch.randn(M, d, generator=g).bfloat16().cuda()
    o = torch.empty(M, d, device="cuda", dtype=torch.bfloat16); dqkv = torch.empty(M, 3 * d, device="cuda", dtype=torch.bfloat16)
    p = torch.zeros(ncap, H, T, T, device="cuda"); km = torch.ones(M, device="cuda")
    a = L.AttnArgs()
    a.precision, a.qkv_dtype, a.o_dtype, a.dqkv_dtype = 1, 1, 1, 1
    a.q, a.k, a.v = qkv.data_ptr(), qkv.data_ptr() + 2 * d, qkv.data_ptr() + 4 * d
    a.o, a.p, a.kmask = o.data_ptr(), p.data_ptr(), km.data_ptr()
    a.ldq = a.ldk = a.ldv = 3 * d; a.ldo = d
    a.nkv, a.H, a.Lq, a.Lk, a.dk, a.causal_period, a.drop_p, a.drop_seed = ncap, H, T, T, dk, T, 0.1, 5
    a.d_o, a.dq, a.d_k, a.dv = do.data_ptr(), dqkv.data_ptr(), dqkv.data_ptr() + 2 * d, dqkv.data_ptr() + 4 * d
    a.lddo = d; a.lddq = a.lddk = a.lddv = 3 * d
    if lengths != [T] * ncap:
        qo = torch.tensor(off, dtype=torch.int32).cuda()
        a.q_off, a.q_off_stride, a.kv_ragged = qo.data_ptr(), 1, 1
    fns = (("fwd", L.lib().ortk_attention_fwd), ("bwd", L.lib().ortk_attention_bwd))
    res, sums = {}, {}
    for rep in range(3):
        for sw in (0, 4, 8):
            L.set_tuning(attn16_short=sw)
            for fname, fn in fns:
                for _ in range(3): L.check(fn(C.byref(a), L.stream_ptr()), fname)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(50): fn(C.byref(a), L.stream_ptr())
                e1.record(); torch.cuda.synchronize()
                res.setdefault((sw, fname), []).append(e0.elapsed_time(e1) * 20)
            sums[sw] = [hashlib.md5(t.cpu().view(torch.int16).numpy().tobytes()).hexdigest() for t in (o, dqkv)] + \
                       [hashlib.md5(p.cpu().numpy().tobytes()).hexdigest()]
    L.set_tuning(attn16_short=1)
    for sw in (0, 4, 8):
        print(f"{name:8s} attn16_short={sw}: fwd us {' '.join(f'{x:6.1f}' for x in res[(sw, 'fwd')])}   bwd us {' '.join(f'{x:6.1f}' for x in res[(sw, 'bwd')])}"
              f"   outputs {'== attn16_short=0' if sums[sw] == sums[0] else 'DIFFER'}", flush=True)


case("padded", [T] * ncap)
gl = torch.Generator().manual_seed(11)
case("valid", torch.randint(9, T + 1, (ncap,), generator=gl).tolist())
