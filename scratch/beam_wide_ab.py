"""Beam decodes of 256 images (36 regions, vocabulary 10 001, mixed precision, the executor `auto` picks):
  (1) width 5 and (2) width 8 on the narrow selection step, (3) width 8 with `stack_debug=64` (the wide step on the same logits),
  (4) width 10, (5) width 16, (6) width 32 (the wide step).
Every arm is a fresh process: `--warmup` decodes, then `--decodes` decodes, each timed by a host clock around the call and a device
synchronise; the figure of a run is the median, in ms per decode, and the figure of an arm the median of its runs.  The arms run
`--reps` times, interleaved.  Nothing is asserted: the numbers go to profiles/beam_wide.txt (`--out` rewrites the head of the file and
keeps it from the line that starts with NOTES_MARK on).  Kernel times come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scratch/beam_wide_ab.py --arm VARIANT --decodes 4 --warmup 1
(`--arm` is what the parent process starts for every run; VARIANT: b5 | b8 | b8w | b10 | b16 | b32)."""
import argparse, json, os, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTES_MARK = "---- notes"
N_IMG = 256
ARMS = [("1 width 5, narrow step", "b5"), ("2 width 8, narrow step", "b8"), ("3 width 8, stack_debug=64", "b8w"), ("4 width 10", "b10"),
        ("5 width 16", "b16"), ("6 width 32", "b32")]


def arm(variant, decodes, warmup):
    sys.path.insert(0, HERE)
    import torch
    import bench
    import sparse_image_captioning_amd as pkg
    from sparse_image_captioning_amd.utils.config import ort_config
    dev = torch.device("cuda", 0)
    config = ort_config(drop_prob_src=0.5, prune_type="supermask", max_seq_length=18)
    torch.manual_seed(8888)
    model = pkg.get_model("relation_transformer")(config, precision="bf16").to(dev).eval()
    b = bench.synth_batch(N_IMG, 36, config.att_feat_size, config.vocab_size, 5, config.max_seq_length, 1000, dev)
    kw = dict(att_feats=b["att_feats"], boxes=b["boxes"], att_masks=b["att_masks"], mode="sample")
    opt = {"beam_size": int(variant[1:].rstrip("w"))}
    if variant.endswith("w"):
        opt["stack_debug"] = 64
    with torch.no_grad():
        for _ in range(warmup):
            model(**kw, opt=opt)
        res = []
        for _ in range(decodes):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            seq, _ = model(**kw, opt=opt)
            torch.cuda.synchronize(); res.append(round((time.perf_counter() - t0) * 1e3, 4))
    print(json.dumps({"ms": res, "rows": int(seq.size(0) * seq.size(1)), "tokens": int(seq.sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decodes", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=2, help="runs per arm")
    ap.add_argument("--out")
    ap.add_argument("--arm", metavar="VARIANT", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.arm:
        return arm(a.arm, a.decodes, a.warmup)
    runs = {name: [] for name, _ in ARMS}
    for rep in range(a.reps):
        for name, variant in ARMS:       # this process never touches the GPU: one arm, one child
            print(f"run {rep + 1}: {name}", file=sys.stderr, flush=True)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", variant, "--decodes", str(a.decodes), "--warmup", str(a.warmup)],
                               capture_output=True, text=True, timeout=300)
            if r.returncode:
                sys.exit(f"arm '{name}' failed with status {r.returncode}:\n{r.stderr[-2000:]}")       # (nothing more runs on the GPU after a failed arm)
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    lines = [f"beam decode, {N_IMG} images, 36 regions, V 10 001, 18 positions, bf16, executor auto; ms per decode: median of {a.decodes} decodes after "
             f"{a.warmup} warm-up decodes; {a.reps} runs per arm, interleaved, each a fresh process"]
    for name, rs in runs.items():
        meds = [statistics.median(r["ms"]) for r in rs]
        lines.append(f"{name:28s} {statistics.median(meds):8.3f}   runs {' '.join(f'{m:.3f}' for m in meds)}   rows {rs[0]['rows']:5d}   token sum {rs[0]['tokens']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        notes = ""
        if os.path.exists(a.out):
            old = open(a.out).read().splitlines(keepends=True)
            at = [i for i, l in enumerate(old) if l.startswith(NOTES_MARK)]
            notes = "".join(old[at[0]:]) if at else ""
        with open(a.out, "w") as f:
            f.write(text + ("\n" + notes if notes else ""))


if __name__ == "__main__":
    main()
