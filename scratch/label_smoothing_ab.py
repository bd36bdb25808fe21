"""A/B on one box, one session: the XE step of bench.py (configs[1]: 256 images x 5 captions x 36 regions, mixed precision) with
  (1) the plain criterion in a checkout of the PARENT commit (`--parent DIR`: built there with `make -C .../csrc`),
  (2) the plain criterion at this commit (label_smoothing = 0 runs ortk_loss: the same code as (1)),
  (3) the label-smoothed criterion (label_smoothing = 0.1: ortk_loss_smooth) at this commit.
Every arm is a fresh process (two libraries of one name cannot share one), bench.py's warm-up (10 steps), then `--blocks` blocks of
`--steps` steps; the figure of a run is the median over its blocks, in ms per step, and the figure of an arm the median of its runs.
The arms run `--reps` times, interleaved; the spread is the distance between the slowest and the fastest run of (1), and the table
says whether (2) agrees with (1), and whether (3) exceeds (1), by more than that.  `--out FILE` also writes the table to the head
of FILE (profiles/label_smoothing.txt) and keeps whatever FILE holds from the line that starts with NOTES_MARK on."""
import argparse, json, os, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTES_MARK = "---- notes"


def arm(root, smoothing, blocks, steps, warmup):
    sys.path.insert(0, root)
    import torch
    import bench
    import sparse_image_captioning_amd as pkg
    from sparse_image_captioning_amd.utils.config import ort_config
    from sparse_image_captioning_amd.training import NativeTrainer
    assert os.path.dirname(os.path.dirname(os.path.abspath(pkg._lib.LIB_PATH))) == os.path.abspath(root), pkg._lib.LIB_PATH  # this arm's own library
    dev = torch.device("cuda", 0)
    config = ort_config(drop_prob_src=0.5, prune_type="supermask", max_seq_length=18)
    torch.manual_seed(8888)
    model = pkg.get_model("relation_transformer")(config, precision="bf16").to(dev).train()
    batch = bench.synth_batch(256, 36, config.att_feat_size, config.vocab_size, 5, config.max_seq_length, 1000, dev)
    kw = {"label_smoothing": smoothing} if smoothing > 0 else {}        # (the parent's trainer does not know the keyword)
    tr = NativeTrainer(model, noamopt_factor=1.0, noamopt_warmup=20000, **kw)
    for _ in range(warmup): tr.xe_step(batch)
    res = []
    for _ in range(blocks):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(steps): loss = tr.xe_step(batch)
        torch.cuda.synchronize(); res.append(round((time.perf_counter() - t0) * 1e3 / steps, 4))
    print(json.dumps({"ms": res, "loss": float(loss), "abi": pkg._lib.ABI_VERSION}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit (required: the A/B is against the parent)")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3, help="runs per arm (at least 2: the spread is between runs of arm 1)")
    ap.add_argument("--out")
    ap.add_argument("--arm", nargs=2, metavar=("ROOT", "SMOOTHING"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.arm:
        return arm(a.arm[0], float(a.arm[1]), a.blocks, a.steps, a.warmup)
    if not a.parent or not os.path.isdir(a.parent):
        ap.error("--parent DIR (a built checkout of the parent commit) is required")
    if a.reps < 2:
        ap.error("--reps must be at least 2")
    arms = [("1 parent, plain", a.parent, 0.0), ("2 this commit, plain", HERE, 0.0), ("3 this commit, smoothing 0.1", HERE, 0.1)]
    runs = {name: [] for name, _, _ in arms}
    for rep in range(a.reps):
        for name, root, sm in arms:       # this process never touches the GPU: one arm, one child
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", os.path.abspath(root), str(sm), "--blocks", str(a.blocks),
                                  "--steps", str(a.steps), "--warmup", str(a.warmup)], check=True, capture_output=True, text=True, timeout=600).stdout
            runs[name].append(json.loads(out.strip().splitlines()[-1]))
    lines = [f"XE step, B = 256, bf16, ms per step: median of {a.blocks} blocks of {a.steps} steps after {a.warmup} warm-up steps; "
             f"{a.reps} runs per arm, interleaved, each a fresh process"]
    fig = {}
    for name, rs in runs.items():
        meds = [statistics.median(r["ms"]) for r in rs]
        fig[name[0]] = (statistics.median(meds), meds)
        lines.append(f"{name:32s} {fig[name[0]][0]:.3f}   runs {' '.join(f'{m:.3f}' for m in meds)}   "
                     f"last loss {rs[0]['loss']:.5f}  ORTK_VERSION {rs[0]['abi']}")
    spread = max(fig["1"][1]) - min(fig["1"][1])
    d2, d3 = fig["2"][0] - fig["1"][0], fig["3"][0] - fig["1"][0]
    lines.append(f"spread (slowest - fastest run of arm 1): {spread:.3f} ms")
    lines.append(f"(2) - (1) = {d2:+.3f} ms: {'within' if abs(d2) <= spread else 'OUTSIDE'} the spread")
    lines.append(f"(3) - (1) = {d3:+.3f} ms: {'within' if d3 <= spread else 'ABOVE'} the spread")
    for name, rs in runs.items():
        lines.append(f"blocks of arm {name[0]}: " + "  ".join(str(r["ms"]) for r in rs))
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
