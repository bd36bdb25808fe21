"""The joint diverse executor (`executor="unfused_joint"`) against the staggered one (`"unfused"`) on diverse beam decodes of 256 images
(36 regions, vocabulary 10 001, mixed precision), with the plain unfused search of the same width as the floor:
  (1) width 10 plain, (2) width 10 in 5 groups of 2, staggered, (3) the same, joint, (4) width 32 plain, (5) width 32 in 4 groups of 8,
  staggered, (6) the same, joint.
Every arm is a fresh process: `--warmup` decodes, then `--decodes` decodes, each timed by a host clock around the call and a device
synchronise; the figure of a run is the median, in ms per decode, the figure of an arm the median of its runs' medians, its spread
the distance between the smallest and the largest of them.  The arms run `--reps` times, interleaved.  Nothing is asserted: the
numbers go to profiles/diverse_joint.txt (`--out` rewrites the head of the file and keeps it from the line that starts with NOTES_MARK
on).  Kernel launches per decode and the selection kernel's time come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scratch/diverse_joint_ab.py --arm VARIANT --decodes 4 --warmup 1
and `--launches DIR --decodes-traced 5` counts the rows of the trace that run wrote (all kernels / decodes traced) and sums up the
selection kernels.  VARIANT: b10u | b10g5 | b10g5j | b32u | b32g4 | b32g4j."""
import argparse, csv, glob, json, os, re, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTES_MARK = "---- notes"
N_IMG = 256
ARMS = [("1 width 10, plain, unfused", "b10u"), ("2 width 10, 5 groups of 2, staggered", "b10g5"), ("3 width 10, 5 groups of 2, joint", "b10g5j"),
        ("4 width 32, plain, unfused", "b32u"), ("5 width 32, 4 groups of 8, staggered", "b32g4"), ("6 width 32, 4 groups of 8, joint", "b32g4j")]


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
    m = re.fullmatch(r"b(\d+)(u|g(\d+)(j?))", variant)
    opt = {"beam_size": int(m.group(1)), "executor": "unfused"}
    if m.group(3):
        opt["group_size"] = int(m.group(3))
        if m.group(4):
            opt["executor"] = "unfused_joint"
    with torch.no_grad():
        for _ in range(warmup):
            model(**kw, opt=opt)
        res = []
        for _ in range(decodes):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            seq, _ = model(**kw, opt=opt)
            torch.cuda.synchronize(); res.append(round((time.perf_counter() - t0) * 1e3, 4))
    distinct = sum(len({tuple(r) for r in img.tolist()}) for img in seq.cpu()) / seq.size(0)
    print(json.dumps({"ms": res, "rows": int(seq.size(0) * seq.size(1)), "tokens": int(seq.sum()), "distinct": distinct}), flush=True)


def launches(trace_dir, decodes_traced):
    """kernel launches per decode of one profiled `--arm` run, and its selection kernels (beam_step_*), from the kernel trace"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {trace_dir}")
    n, sel = 0, {}
    for f in files:
        for row in csv.DictReader(open(f)):
            n += 1
            name = row.get("Kernel_Name", "")
            if "beam_step" in name:
                short = re.sub(r"\(.*$", "", name.replace("void ortk::(anonymous namespace)::", ""))
                d = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
                s = sel.setdefault(short, [0, 0.0, float("inf"), 0.0])
                s[0] += 1; s[1] += d; s[2] = min(s[2], d); s[3] = max(s[3], d)
    print(f"{n} kernel launches in {decodes_traced} decodes: {n / decodes_traced:.0f} per decode")
    for k, (c, tot, lo, hi) in sorted(sel.items()):
        print(f"  {k}: {c} launches, mean {tot / c:.1f} us (min {lo:.1f}, max {hi:.1f}), {tot / decodes_traced / 1e3:.3f} ms per decode")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decodes", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="runs per arm")
    ap.add_argument("--out")
    ap.add_argument("--arm", metavar="VARIANT", help=argparse.SUPPRESS)
    ap.add_argument("--launches", metavar="DIR", help="count the launches of a profiled --arm run")
    ap.add_argument("--decodes-traced", type=int, default=5)
    a = ap.parse_args()
    if a.arm:
        return arm(a.arm, a.decodes, a.warmup)
    if a.launches:
        return launches(a.launches, a.decodes_traced)
    runs = {name: [] for name, _ in ARMS}
    for rep in range(a.reps):
        for name, variant in ARMS:       # this process never touches the GPU: one arm, one child
            print(f"run {rep + 1}: {name}", file=sys.stderr, flush=True)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", variant, "--decodes", str(a.decodes), "--warmup", str(a.warmup)],
                               capture_output=True, text=True, timeout=300)
            if r.returncode:
                sys.exit(f"arm '{name}' failed with status {r.returncode}:\n{r.stderr[-2000:]}")       # (nothing more runs on the GPU after a failed arm)
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    lines = [f"beam decode, {N_IMG} images, 36 regions, V 10 001, 18 positions, bf16; ms per decode: median of {a.decodes} decodes after "
             f"{a.warmup} warm-up decodes; {a.reps} runs per arm, interleaved, each a fresh process; arm = median of the runs' medians, spread = max - min of them"]
    for name, rs in runs.items():
        meds = [statistics.median(r["ms"]) for r in rs]
        lines.append(f"{name:38s} {statistics.median(meds):8.3f}   spread {max(meds) - min(meds):6.3f}   runs {' '.join(f'{m:.3f}' for m in meds)}   rows {rs[0]['rows']:5d}   "
                     f"distinct captions per image {rs[0]['distinct']:.2f}   token sum {rs[0]['tokens']}")
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
