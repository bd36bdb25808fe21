"""SCST step with the REAL reward: host CaptionScorer against the device scorer (profiles/scst_device_reward.txt).

    python scratch/scst_device_reward.py [--steps 10 --rounds 3 --warmup 4] > profiles/scst_device_reward.txt

Shape of BASELINE configs[3] as bench.py times it (256 images, 5 train-mode rollouts + eval-mode greedy, random-init model with
the `hostreward` variant's generator scaling so captions end), 5 synthetic references per image of 8-16 tokens, CIDEr-D with a
cached document-frequency table in token-id space.
  (a) scst_step with the host scorer_reward_fn (the code path of the parent commit: this change does not touch it)
  (b) scst_step with scorer_reward_fn(device=True), and the scorer kernel alone (HIP events)
  (c) host time of device_refs (pack + upload) for one batch
(a) and (b) alternate in blocks inside one process; every step ends in a device synchronise."""
import argparse
import hashlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    return f"min {min(ms):.3f}  median {float(np.median(ms)):.3f}  max {max(ms):.3f} ms  (n = {len(ms)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="steps per block")
    ap.add_argument("--rounds", type=int, default=3, help="alternating blocks per variant")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--eos-bias", type=float, default=5.4)
    args = ap.parse_args()
    import bench
    import sparse_image_captioning_amd as pkg
    from sparse_image_captioning_amd.scst import CaptionScorer
    from sparse_image_captioning_amd.training import NativeTrainer
    from sparse_image_captioning_amd.utils.config import ort_config
    pkg._lib.require_gpu()
    dev = torch.device("cuda:0")
    B, ns, S = 256, 5, 36
    config = ort_config(drop_prob_src=0.5, prune_type="supermask", max_seq_length=18)
    torch.manual_seed(8888)
    model = pkg.get_model("relation_transformer")(config, precision="bf16")
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if n_.endswith("generator.proj.weight"):
                p.mul_(3.0)
            if n_.endswith("generator.proj.bias"):
                p[config.eos_token_id] += args.eos_bias
    model = model.to(dev).train()
    batch = bench.synth_batch(B, S, config.att_feat_size, config.vocab_size, 5, config.max_seq_length, 1000, dev)
    rs = np.random.RandomState(7)
    # (references over the whole vocabulary: a random-init model rarely shares an n-gram with them, most rewards are 0 —
    # the scorers do the same work either way: every hypothesis n-gram is looked up)
    refs = [[[int(t) for t in rs.randint(4, config.vocab_size, size=rs.randint(8, 17))] for _ in range(5)] for _ in range(B)]
    grams = sorted({tuple(c[i:i + k]) for r in refs for c in r for k in range(1, 5) for i in range(len(c) - k + 1)})
    table = {"document_frequency": {g: float(c) for g, c in zip(grams, rs.randint(1, 400, size=len(grams)))}, "ref_len": 5000.0}
    scorer = CaptionScorer(table, cider_weight=1.0)
    tr = NativeTrainer(model, noamopt_factor=1.0, noamopt_warmup=20000)
    host_fn = NativeTrainer.scorer_reward_fn(scorer, refs, eos_idx=config.eos_token_id, pad_idx=config.pad_token_id)
    t0 = time.perf_counter()
    drefs = scorer.device_refs(refs, ns + 1, dev, vocab_size=config.vocab_size)       # (first call: also serialises + uploads the df table)
    torch.cuda.synchronize()
    first_refs_ms = (time.perf_counter() - t0) * 1e3
    dev_fn = NativeTrainer.scorer_reward_fn(scorer, drefs, eos_idx=config.eos_token_id, pad_idx=config.pad_token_id, device=True,
                                            vocab_size=config.vocab_size)
    last = {}

    def step(fn, valid_positions=True):
        tr.valid_positions = valid_positions
        torch.cuda.synchronize()
        t = time.perf_counter()
        last["res"] = tr.scst_step(batch, fn, num_samples=ns, baseline="greedy")
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    variants = {"a_host": (host_fn, True), "a_host_padded": (host_fn, False), "b_device": (dev_fn, True)}
    for _ in range(args.warmup):
        for fn, vp in variants.values():
            step(fn, vp)
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, (fn, vp) in variants.items():
            times[k] += [step(fn, vp) for _ in range(args.steps)]
    loss, reward, seq, greedy = last["res"]
    # the two rewards on the last step's tokens
    r_host = host_fn(seq, greedy).numpy()
    r_dev = dev_fn(seq, greedy).cpu().numpy()
    lens = (seq != config.pad_token_id).sum(-1).float()
    # host scorer alone on those tokens (D2H copy + Python row loop + native scorer)
    host_alone = []
    for _ in range(10):
        t = time.perf_counter()
        host_fn(seq, greedy)
        host_alone.append((time.perf_counter() - t) * 1e3)
    # kernel alone: HIP events around 20 launches, 5 repeats
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kern = []
    for _ in range(3):
        scorer.score_device(drefs, seq, greedy, eos_idx=config.eos_token_id, pad_idx=config.pad_token_id)
    for _ in range(5):
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(20):
            scorer.score_device(drefs, seq, greedy, eos_idx=config.eos_token_id, pad_idx=config.pad_token_id)
        ev[1].record()
        torch.cuda.synchronize()
        kern.append(ev[0].elapsed_time(ev[1]) / 20)
    # (c) device_refs for one batch
    pack_ms, refs_ms = [], []
    for _ in range(10):
        t = time.perf_counter()
        hp = scorer.pack_refs(refs, ns + 1)
        pack_ms.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        scorer.device_refs(hp, ns + 1, dev)
        torch.cuda.synchronize()
        refs_ms.append((time.perf_counter() - t) * 1e3)
    corpus = CaptionScorer("corpus", cider_weight=1.0)
    corpus_ms = []
    for _ in range(10):
        t = time.perf_counter()
        corpus.device_refs(refs, ns + 1, dev)
        torch.cuda.synchronize()
        corpus_ms.append((time.perf_counter() - t) * 1e3)

    md5 = hashlib.md5(open(pkg._lib.LIB_PATH, "rb").read()).hexdigest()
    print(f"libortk.so md5 {md5}")
    print(f"device {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {B} images x ({ns} samples + greedy), L = {config.max_seq_length}, "
          f"bf16 storage, 5 references per image of 8-16 tokens, cached df table of {len(grams)} n-grams; {hp.pack.size} B pack, "
          f"{hp.df.size} B df table")
    print(f"sampled captions: mean {float(lens.mean()):.2f} non-pad positions (EOS included), {float((lens == config.max_seq_length).float().mean()) * 100:.1f} % of the rows use all {config.max_seq_length}")
    print(f"reward on the last step's tokens: host vs device max abs diff {float(np.abs(r_host - r_dev).max()):.3e}; "
          f"{float((np.abs(r_host) > 0).mean()) * 100:.1f} % non-zero")
    print(f"warm-up {args.warmup} steps per variant, then {args.rounds} alternating blocks of {args.steps} steps; host clock around a step that ends in a device synchronise")
    print(f"(a)  scst_step, host scorer_reward_fn (valid-position update)   {stats(times['a_host'])}")
    print(f"(a') scst_step, host scorer_reward_fn, padded update            {stats(times['a_host_padded'])}")
    print(f"(b)  scst_step, scorer_reward_fn(device=True) (padded update)   {stats(times['b_device'])}")
    ma, mb = float(np.median(times["a_host"])), float(np.median(times["b_device"]))
    print(f"gain (a) -> (b): {ma - mb:+.3f} ms per step ({(ma / mb - 1) * 100:+.1f} % steps/s), medians")
    print(f"host reward_fn alone (D2H copy, Python row loop, native scorer, on this host)  {stats(host_alone)}")
    print(f"scorer kernel alone (HIP events, 20 launches per sample)                       {stats(kern)}")
    print(f"(c)  pack_refs on the host, cached mode                                        {stats(pack_ms)}")
    print(f"(c)  device_refs from that pack (pin + upload + synchronise)                   {stats(refs_ms)}")
    print(f"(c)  device_refs, corpus mode (cook + batch df table + upload + synchronise)   {stats(corpus_ms)}")
    print(f"first device_refs of the scorer (also serialises and uploads the df table)     {first_refs_ms:.3f} ms")


if __name__ == "__main__":
    main()
