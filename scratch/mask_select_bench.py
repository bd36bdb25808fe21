"""Mask selection at full size: the torch route (cat + topk + scatter) against `select="device"` (ortk_mask_select).

    python scratch/mask_select_bench.py [--reps 5 --warmup 2 --target 0.95] > profiles/mask_select.txt

The prune model at BASELINE configs[2] geometry (55.4 M parameters, every >= 2-D weight maskable, xavier init), one-shot update at
the target for mag_blind, mag_uniform and mag_dist.  Per route: HIP events around `update_masks_once` and around the selection
alone (warm-up first; the two routes alternate), and the peak of `torch.cuda.max_memory_allocated` above what is resident before the call (model, masks, and for the
device route its cached tables and workspace, which are listed separately).  The bytes the device route moves are counted from
the pass structure of csrc/ortk_select.hip: 6 reads of the active weights + 1 mask write (kind 1: 8 reads)."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    return f"min {min(ms):9.3f}  median {float(np.median(ms)):9.3f}  max {max(ms):9.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--target", type=float, default=0.95)
    args = ap.parse_args()
    import sparse_image_captioning_amd as pkg
    from sparse_image_captioning_amd.pruning import prune
    from sparse_image_captioning_amd.utils.config import ort_config
    pkg._lib.require_gpu()
    dev = torch.device("cuda:0")
    md5 = hashlib.md5(open(pkg._lib.LIB_PATH, "rb").read()).hexdigest()
    print(f"libortk.so md5 {md5}")
    print(f"device {torch.cuda.get_device_name(0)}; torch {torch.__version__}; target {args.target}; warm-up {args.warmup}, then "
          f"{args.reps} alternating repetitions per route; HIP events around update_masks_once; MB = 1e6 bytes")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    @torch.no_grad()
    def selection_only(model, select):
        """The selection without `sparsity_check()` (147 host-synchronising sums that both routes share)."""
        if select == "device":
            return model._select_masks_device(args.target)
        masks, weights = model.active_pruning_masks(named=False), model.active_pruned_weights(named=False)
        fresh = [model.compute_mask(c, args.target) for c in prune._rank_by(model.mask_type, weights, masks)]
        if len(fresh) == 1:
            fresh = torch.split(fresh[0], [m.nelement() for m in masks])
        for m, f in zip(masks, fresh):
            m.data.view(-1).copy_(f.reshape(-1))

    def timed(model, select, whole=True):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ev[0].record()
        if whole:
            model.update_masks_once(args.target, select=select)
        else:
            selection_only(model, select)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), torch.cuda.max_memory_allocated() - base

    for mask_type in ("mag_blind", "mag_uniform", "mag_dist"):
        torch.manual_seed(8888)
        model = pkg.get_model("relation_transformer_prune")(ort_config(prune_type=mask_type)).to(dev).eval()
        n = sum(m.numel() for m in model.active_pruning_masks(named=False))
        resident = torch.cuda.memory_allocated()
        out = {}
        for select in ("torch", "device"):
            for _ in range(args.warmup):
                timed(model, select)
        plan = model._select_plan()
        plan_bytes = plan["ws"].numel() + sum(t.numel() * 8 for t in plan["tables"])
        times, peaks, alone = {"torch": [], "device": []}, {"torch": [], "device": []}, {"torch": [], "device": []}
        for _ in range(args.reps):
            for select in ("torch", "device"):
                alone[select].append(timed(model, select, whole=False)[0])
                ms, peak = timed(model, select)
                times[select].append(ms)
                peaks[select].append(peak)
                out[select] = torch.cat([m.detach().reshape(-1) for m in model.active_pruning_masks(named=False)]).clone()
        n_seg, n_groups, n_chunks, kind = plan["counts"]
        moved = (6 + 2 * kind + 1) * 4 * n
        differ = int((out["torch"] != out["device"]).sum())
        kept = {k: int(v.sum()) for k, v in out.items()}
        why = "equal criteria at the threshold" if kind == 0 else "criteria at the threshold: equal ones, and fp32 vs fp64 mean / std"
        print(f"\n{mask_type}: {n} active weights in {n_seg} segments, {n_groups} group(s), {n_chunks} chunks; model + masks resident "
              f"{resident / 1e6:.1f} MB")
        print(f"  torch route    {stats(times['torch'])}   peak transient {max(peaks['torch']) / 1e6:9.1f} MB")
        print(f"  device route   {stats(times['device'])}   peak transient {max(peaks['device']) / 1e6:9.1f} MB   "
              f"(+ {plan_bytes / 1e3:.1f} kB of cached tables and workspace)")
        print(f"  selection only, torch    {stats(alone['torch'])}   (the same without sparsity_check(): 147 sums that synchronise the host)")
        print(f"  selection only, device   {stats(alone['device'])}")
        med = float(np.median(alone["device"]))
        print(f"  device route moves {moved / 1e6:.1f} MB per call ({6 + 2 * kind} reads + 1 write of the active weights): "
              f"{moved / med / 1e6:.1f} GB/s over the median selection (launches and the n_drop upload included)")
        print(f"  selection only, median torch / median device = {float(np.median(alone['torch'])) / med:.1f}x;  kept entries torch {kept['torch']}, "
              f"device {kept['device']};  positions where the two masks differ: {differ} ({why})")
        del model, out, plan
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
