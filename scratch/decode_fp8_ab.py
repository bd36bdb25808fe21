"""A/B on one box, one session: the beam-5 decode of bench.py's decode workload (ORT dense, 36 regions, mixed precision) at 1 024 and at
320 images with
  (1) `executor="stack"` in a checkout of the PARENT commit (`--parent DIR`: built there with `make -C .../csrc`),
  (2) `executor="stack"` at this commit (the same kernel: its resource report is unchanged),
  (3) `executor="stack_fp8"` at this commit (the FP8 weight stream, ORTK_DEC_STACK_FP8).
Every arm is a fresh process (two libraries of one name cannot share one): `--warmup` decodes, then `--decodes` decodes, each timed by
a host clock around the call and a device synchronise; the figure of a run is the median, in ms per decode, and the figure of an arm
the median of its runs.  The arms run `--reps` times, interleaved; the spread is the distance between the slowest and the fastest run
of (1).  After the timed decodes one more runs under the library's own profiler (ortk_prof_enable: device events around the stack
kernel's launches) and gives the kernel's us per position.  Nothing is asserted: the numbers go to profiles/decode_fp8.txt (`--out`
rewrites the head of the file and keeps it from the line that starts with NOTES_MARK on)."""
import argparse, ctypes, json, os, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTES_MARK = "---- notes"


def arm(root, executor, n_img, decodes, warmup):
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
    b = bench.synth_batch(n_img, 36, config.att_feat_size, config.vocab_size, 5, config.max_seq_length, 1000, dev)
    kw = dict(att_feats=b["att_feats"], boxes=b["boxes"], att_masks=b["att_masks"], mode="sample")
    opt = {"beam_size": 5, "executor": executor}
    with torch.no_grad():
        for _ in range(warmup):
            model(**kw, opt=opt)
        res = []
        for _ in range(decodes):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            seq, _ = model(**kw, opt=opt)
            torch.cuda.synchronize(); res.append(round((time.perf_counter() - t0) * 1e3, 4))
        L.lib().ortk_prof_enable(2)
        try:
            model(**kw, opt=opt)
            torch.cuda.synchronize()
            n, ms, fl = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
            L.check(L.lib().ortk_prof_collect(16, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl)), "ortk_prof_collect")       # PROF_KEY_DECSTACK
        finally:
            L.lib().ortk_prof_enable(0)
    print(json.dumps({"ms": res, "stack_us_per_position": round(ms.value * 1e3 / max(n.value, 1), 2), "positions": n.value,
                      "tokens": int(seq.sum()), "abi": L.ABI_VERSION}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit (required: the A/B is against the parent)")
    ap.add_argument("--decodes", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=2, help="runs per arm (at least 2: the spread is between runs of arm 1)")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 320])
    ap.add_argument("--out")
    ap.add_argument("--arm", nargs=3, metavar=("ROOT", "EXECUTOR", "IMAGES"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.arm:
        return arm(a.arm[0], a.arm[1], int(a.arm[2]), a.decodes, a.warmup)
    if not a.parent or not os.path.isdir(a.parent):
        ap.error("--parent DIR (a built checkout of the parent commit) is required")
    if a.reps < 2 or a.decodes < 20:
        ap.error("--reps must be at least 2 and --decodes at least 20")
    arms = [("1 parent, stack", a.parent, "stack"), ("2 this commit, stack", HERE, "stack"), ("3 this commit, stack_fp8", HERE, "stack_fp8")]
    lines = []
    for n_img in a.sizes:
        runs = {name: [] for name, _, _ in arms}
        for rep in range(a.reps):
            for name, root, ex in arms:       # this process never touches the GPU: one arm, one child
                print(f"{n_img} images, run {rep + 1}: {name}", file=sys.stderr, flush=True)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", os.path.abspath(root), ex, str(n_img), "--decodes", str(a.decodes),
                                    "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=300)
                if r.returncode:
                    sys.exit(f"arm '{name}' failed with status {r.returncode}:\n{r.stderr[-2000:]}")       # (nothing more runs on the GPU after a failed arm)
                out = r.stdout
                runs[name].append(json.loads(out.strip().splitlines()[-1]))
        lines.append(f"beam-5 decode, {n_img} images x 36 regions, bf16, ms per decode: median of {a.decodes} decodes after {a.warmup} warm-up decodes; "
                     f"{a.reps} runs per arm, interleaved, each a fresh process")
        fig = {}
        for name, rs in runs.items():
            meds = [statistics.median(r["ms"]) for r in rs]
            fig[name[0]] = (statistics.median(meds), meds)
            lines.append(f"{name:28s} {fig[name[0]][0]:8.3f}   runs {' '.join(f'{m:.3f}' for m in meds)}   stack kernel us per position "
                         f"{' '.join(str(r['stack_us_per_position']) for r in rs)} ({rs[0]['positions']} launches)   token sum {rs[0]['tokens']}  ORTK_VERSION {rs[0]['abi']}")
        spread = max(fig["1"][1]) - min(fig["1"][1])
        lines.append(f"spread (slowest - fastest run of arm 1): {spread:.3f} ms;  (2) - (1) = {fig['2'][0] - fig['1'][0]:+.3f} ms;  (3) - (2) = {fig['3'][0] - fig['2'][0]:+.3f} ms")
        lines.append("")
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
