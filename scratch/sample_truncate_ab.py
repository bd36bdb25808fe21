"""A/B on one box, one session: the multinomial decode of an SCST rollout — 256 images x (5 samples + 1 greedy row) = 1 536 rows,
36 regions, vocabulary 10 001, mixed precision, eval mode, the executor `auto` picks — with
  (1) the plain decode in a checkout of the PARENT commit (`--parent DIR`: built there with `make -C .../csrc`),
  (2) the plain decode at this commit (the same kernels: the generator's sampling epilogue, no logit rows),
  (3) the plain decode with `set_tuning(samp_epilogue=0)`: logit rows stored, sample_step_fused_kernel reads them back,
  (4) `sample_method="top5"` and (5) `sample_method="top0.9"`: logit rows stored, sample_step_trunc_kernel reads them back.
Every arm is a fresh process (two libraries of one name cannot share one): `--warmup` decodes, then `--decodes` decodes, each timed by
a host clock around the call and a device synchronise; the figure of a run is the median, in ms per decode, and the figure of an arm
the median of its runs.  The arms run `--reps` times, interleaved; the spread is the distance between the slowest and the fastest run
of (1).  Nothing is asserted: the numbers go to profiles/sample_truncate.txt (`--out` rewrites the head of the file and keeps it from
the line that starts with NOTES_MARK on).  Kernel times come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scratch/sample_truncate_ab.py --arm ROOT VARIANT --decodes 4 --warmup 1
(`--arm` is what the parent process starts for every run; VARIANT: plain | noepi | top5 | top0.9)."""
import argparse, json, os, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTES_MARK = "---- notes"
N_IMG, N_SAMPLES = 256, 5


def arm(root, variant, decodes, warmup):
    sys.path.insert(0, root)
    import torch
    import bench
    import sparse_image_captioning_amd as pkg
    from sparse_image_captioning_amd.utils.config import ort_config
    assert os.path.dirname(os.path.dirname(os.path.abspath(pkg._lib.LIB_PATH))) == os.path.abspath(root), pkg._lib.LIB_PATH  # this arm's own library
    L = pkg._lib
    dev = torch.device("cuda", 0)
    config = ort_config(drop_prob_src=0.5, prune_type="supermask", max_seq_length=18)
    torch.manual_seed(8888)
    model = pkg.get_model("relation_transformer")(config, precision="bf16").to(dev).eval()
    b = bench.synth_batch(N_IMG, 36, config.att_feat_size, config.vocab_size, 5, config.max_seq_length, 1000, dev)
    kw = dict(att_feats=b["att_feats"], boxes=b["boxes"], att_masks=b["att_masks"], mode="sample")
    opt = {"num_random_sample": N_SAMPLES, "beam_size": 0, "with_greedy": True, "seed": 4242}
    if variant == "noepi":
        L.set_tuning(samp_epilogue=0)
    elif variant != "plain":
        opt["sample_method"] = variant
    with torch.no_grad():
        for _ in range(warmup):
            model(**kw, opt=opt)
        res = []
        for _ in range(decodes):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            seq, _ = model(**kw, opt=opt)
            torch.cuda.synchronize(); res.append(round((time.perf_counter() - t0) * 1e3, 4))
    print(json.dumps({"ms": res, "rows": int(seq.size(0) * seq.size(1)), "tokens": int(seq.sum()), "abi": L.ABI_VERSION}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit (required: the A/B is against the parent)")
    ap.add_argument("--decodes", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=2, help="runs per arm (at least 2: the spread is between runs of arm 1)")
    ap.add_argument("--out")
    ap.add_argument("--arm", nargs=2, metavar=("ROOT", "VARIANT"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.arm:
        return arm(a.arm[0], a.arm[1], a.decodes, a.warmup)
    if not a.parent or not os.path.isdir(a.parent):
        ap.error("--parent DIR (a built checkout of the parent commit) is required")
    if a.reps < 2 or a.decodes < 20:
        ap.error("--reps must be at least 2 and --decodes at least 20")
    arms = [("1 parent, plain", a.parent, "plain"), ("2 this commit, plain", HERE, "plain"), ("3 this commit, samp_epilogue=0", HERE, "noepi"),
            ("4 this commit, top5", HERE, "top5"), ("5 this commit, top0.9", HERE, "top0.9")]
    runs = {name: [] for name, _, _ in arms}
    for rep in range(a.reps):
        for name, root, variant in arms:       # this process never touches the GPU: one arm, one child
            print(f"run {rep + 1}: {name}", file=sys.stderr, flush=True)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", os.path.abspath(root), variant, "--decodes", str(a.decodes),
                                "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=300)
            if r.returncode:
                sys.exit(f"arm '{name}' failed with status {r.returncode}:\n{r.stderr[-2000:]}")       # (nothing more runs on the GPU after a failed arm)
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    rows = runs[arms[0][0]][0]["rows"]
    lines = [f"multinomial decode, {N_IMG} images x ({N_SAMPLES} samples + 1 greedy row) = {rows} rows, 36 regions, V 10 001, bf16, eval mode, executor auto; "
             f"ms per decode: median of {a.decodes} decodes after {a.warmup} warm-up decodes; {a.reps} runs per arm, interleaved, each a fresh process"]
    fig = {}
    for name, rs in runs.items():
        meds = [statistics.median(r["ms"]) for r in rs]
        fig[name[0]] = (statistics.median(meds), meds)
        lines.append(f"{name:32s} {fig[name[0]][0]:8.3f}   runs {' '.join(f'{m:.3f}' for m in meds)}   token sum {rs[0]['tokens']}  ORTK_VERSION {rs[0]['abi']}")
    spread = max(fig["1"][1]) - min(fig["1"][1])
    lines.append(f"spread (slowest - fastest run of arm 1): {spread:.3f} ms;  (2) - (1) = {fig['2'][0] - fig['1'][0]:+.3f} ms;  (3) - (2) = "
                 f"{fig['3'][0] - fig['2'][0]:+.3f} ms;  (4) - (3) = {fig['4'][0] - fig['3'][0]:+.3f} ms;  (5) - (3) = {fig['5'][0] - fig['3'][0]:+.3f} ms")
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
