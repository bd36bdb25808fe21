"""us per launch of every ortk_optim_step kind over the full 55.4 M-element arena, next to ortk_adam_clip_zero, same sitting."""
import ctypes as Ct, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import sparse_image_captioning_amd as pkg
L = pkg._lib
L.require_gpu()
lib = L.lib()
n = 55_443_777
torch.manual_seed(0)
p = torch.randn(n, device="cuda") * 0.1
g = torch.randn(n, device="cuda") * 0.01
s1 = torch.zeros(n, device="cuda"); s2 = torch.zeros(n, device="cuda")
st = L.stream_ptr()
def opt_call(kind):
    k = L.OptimArgs()
    k.p, k.g, k.s1, k.s2, k.n = p.data_ptr(), g.data_ptr(), s1.data_ptr(), s2.data_ptr(), n
    k.kind, k.first_step, k.zero_grad = L.OPT_KINDS[kind], 0, 1
    k.lr, k.weight_decay, k.alpha, k.beta, k.eps, k.clip, k.bc1, k.bc2 = 1e-6, 1e-2, 0.9, 0.999, 1e-8, 0.1, 0.5, 0.5
    return lambda: L.check(lib.ortk_optim_step(Ct.byref(k), st), kind)
calls = {"ortk_adam_clip_zero": lambda: L.check(lib.ortk_adam_clip_zero(L.ptr(p), L.ptr(g), L.ptr(s1), L.ptr(s2), n, 1e-6, 0.9, 0.999, 1e-8, 0.1, 0.5, 0.5, st), "adam")}
for kind in ("adam", "sgd", "sgdm", "sgdmom", "rmsprop", "adagrad"):
    calls["optim_step " + kind] = opt_call(kind)
# arrays read + written per element (zero_grad on: g is read and written)
arrays = {"ortk_adam_clip_zero": 8, "optim_step adam": 8, "optim_step sgd": 4, "optim_step sgdm": 6, "optim_step sgdmom": 6, "optim_step rmsprop": 6, "optim_step adagrad": 6}
res = {k: [] for k in calls}
for rnd in range(5):
    for name, fn in calls.items():
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(40):
            fn()
        b.record(); torch.cuda.synchronize()
        res[name].append(a.elapsed_time(b) * 1000 / 40)
print(f"n = {n} fp32 elements, zero_grad on, 5 rounds x 40 launches per entry (device events), entries interleaved per round")
print(f"{'entry':24s} {'arrays':>6s} {'median us':>10s} {'min':>8s} {'max':>8s} {'GB/s (median)':>14s}")
for name, v in res.items():
    med = statistics.median(v)
    print(f"{name:24s} {arrays[name]:6d} {med:10.1f} {min(v):8.1f} {max(v):8.1f} {arrays[name] * 4 * n / med / 1e3:14.0f}")
