"""A/B of the LayerNorm backward's da / db inside the XE step of bench.py (256 images x 5 captions, bf16), one process, interleaved:
ortk_tuning.ln_fuse = 16 (every workgroup adds its column sums with atomics) against 0 (block partials + one reduce launch per half of
the backward on the third queue).  Three rounds of 20 steps each.

  python scratch/ln_step_ab.py [field=value,field=value ...]      other ortk_tuning settings to interleave, e.g. ln_fuse=0,wgrad_group_wgs=112"""
import ctypes as C, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
import sparse_image_captioning_amd as pkg
from sparse_image_captioning_amd.utils.config import ort_config
from sparse_image_captioning_amd.training import NativeTrainer
L = pkg._lib
dev = torch.device("cuda", 0)
config = ort_config(drop_prob_src=0.5, prune_type="supermask", max_seq_length=18)
torch.manual_seed(8888)
model = pkg.get_model("relation_transformer")(config, precision="bf16").to(dev).train()
batch = bench.synth_batch(256, 36, 2048, 10001, 5, 18, 1000, dev)
tr = NativeTrainer(model, noamopt_factor=1.0, noamopt_warmup=20000)
prev = L.set_tuning()
combos = [dict(ln_fuse=16), dict(ln_fuse=0)]
if len(sys.argv) > 1:
    combos = [{kv.split("=")[0]: int(kv.split("=")[1]) for kv in a.split(",")} for a in sys.argv[1:]]
res = {i: [] for i in range(len(combos))}
try:
    for kw in combos:
        L.set_tuning(**dict(prev, **kw))
        for _ in range(4): tr.xe_step(batch)
    for rep in range(3):
        for i, kw in enumerate(combos):
            L.set_tuning(**dict(prev, **kw))
            for _ in range(2): tr.xe_step(batch)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(20): tr.xe_step(batch)
            torch.cuda.synchronize(); res[i].append((time.perf_counter() - t0) * 50)
finally:
    L.set_tuning(**prev)
for i, kw in enumerate(combos):
    print(",".join(f"{k}={v}" for k, v in kw.items()) + ": " + " ".join(f"{x:.3f}" for x in res[i]) + f" ms per step (mean {sum(res[i]) / 3:.3f})", flush=True)
