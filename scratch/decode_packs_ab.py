"""A/B on one box, one session: prepared decode weights (`model.decode_packs`) on four workloads

  dense1024   the beam-5 decode of bench.py's decode workload (ORT dense, 1 024 images x 36 regions, mixed precision)
  sparse1024  BASELINE configs[4]: the same decode on 95 % zeros through the sparse weight stream (`enable_sparse_stream`)
  dense50     a 50-image beam-5 decode
  steps100    an 18-position `get_logprobs_state` loop at 100 rows (encode + memory projection + 18 steps)

with (1) a checkout of the PARENT commit (`--parent DIR`, built there), (2) this commit with packs off, (3) "cached", (4) "verified".
The parent is a fresh process (two libraries of one name cannot share one).  Arms (2)-(4) ALTERNATE inside one process: decode i runs
variant i mod 3 on one model, so drift of the box falls on all of them alike.  Each is timed by a host clock around the call and a
device synchronise; the figure of a run is the median in ms over `--decodes` timed calls per variant after `--warmup` calls each, the
figure of an arm the median of its `--reps` runs; the spread is the distance between the slowest and the fastest run of (1).  A last
section times ortk_params_fingerprint beside ortk_cast_bf16 on the same arena (device events, median of 50) and the host cost of the
key of the weights (`model._packs_key()`, walked once per call with packs on).  Nothing is asserted:
with `--out profiles/decode_packs.txt` the numbers go to that file (its head is rewritten, the part from the NOTES_MARK line on is
kept).  Not run yet: no figure of it is recorded anywhere."""
import argparse, ctypes, hashlib, json, os, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTES_MARK = "---- notes"
WORKLOADS = ("dense1024", "sparse1024", "dense50", "steps100")


def build(root, workload):
    sys.path.insert(0, root)
    import torch
    import bench
    import sparse_image_captioning_amd as pkg
    from sparse_image_captioning_amd.utils.config import ort_config
    assert os.path.dirname(os.path.dirname(os.path.abspath(pkg._lib.LIB_PATH))) == os.path.abspath(root), pkg._lib.LIB_PATH  # this arm's own library
    dev = torch.device("cuda", 0)
    config = ort_config(drop_prob_src=0.5, prune_type="supermask", max_seq_length=18)
    torch.manual_seed(8888)
    model = pkg.get_model("relation_transformer")(config, precision="bf16").to(dev).eval()
    if workload == "sparse1024":
        with torch.no_grad():
            for p in model.parameters():
                if p.dim() >= 2:
                    p.mul_((torch.rand_like(p) < 0.05).float())
        model.enable_sparse_stream(True)
    n_img = {"dense1024": 1024, "sparse1024": 1024, "dense50": 50, "steps100": 100}[workload]
    b = bench.synth_batch(n_img, 36, config.att_feat_size, config.vocab_size, 5, config.max_seq_length, 1000, dev)
    if workload == "steps100":
        def call():
            mem = model.encode(b["att_feats"], b["boxes"], b["att_masks"])
            amask = b["att_masks"][:, None, :mem.size(1)]
            it = torch.full((mem.size(0),), config.bos_token_id, dtype=torch.long, device=dev)
            state = None
            for _ in range(18):
                lp, state = model.get_logprobs_state(it, mem, amask, state)
                it = lp.argmax(-1)
            return it
    else:
        kw = dict(att_feats=b["att_feats"], boxes=b["boxes"], att_masks=b["att_masks"], mode="sample")

        def call():
            return model(**kw, opt={"beam_size": 5})[0]
    return torch, pkg, model, call


def arm(root, workload, variants, decodes, warmup):
    torch, pkg, model, call = build(root, workload)
    res = {v: [] for v in variants}
    with torch.no_grad():
        for i in range((warmup + decodes) * len(variants)):
            v = variants[i % len(variants)]
            if v != "parent":
                model.decode_packs = None if v == "off" else v
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = call()
            torch.cuda.synchronize(); dt = (time.perf_counter() - t0) * 1e3
            if i >= warmup * len(variants):
                res[v].append(round(dt, 4))
    md5 = hashlib.md5(open(pkg._lib.LIB_PATH, "rb").read()).hexdigest()
    print(json.dumps({"ms": res, "tokens": int(out.sum()), "abi": pkg._lib.ABI_VERSION, "md5": md5}), flush=True)


def fingerprint_cost(root):
    torch, pkg, model, _ = build(root, "dense50")
    L = pkg._lib
    n = model._n_train
    w16 = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(1, dtype=torch.int64, device="cuda")
    runs = {"ortk_cast_bf16": lambda: L.lib().ortk_cast_bf16(L.ptr(model._flat), L.ptr(w16), n, L.stream_ptr()),
            "ortk_params_fingerprint": lambda: L.lib().ortk_params_fingerprint(L.ptr(model._flat), n, L.ptr(out), L.stream_ptr())}
    fig = {}
    for name, fn in runs.items():
        for _ in range(5):
            fn()
        ts = []
        for _ in range(50):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        fig[name] = round(statistics.median(ts), 1)
    t0 = time.perf_counter()                     # host side: the key of the weights, walked once per call with packs on
    for _ in range(2000):
        model._packs_key()
    key_us = round((time.perf_counter() - t0) / 2000 * 1e6, 1)
    print(json.dumps({"n": n, "us": fig, "key_us": key_us, "n_par": len(list(model.parameters()))}), flush=True)


def child(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode:
        sys.exit(f"child {args} failed with status {r.returncode}:\n{r.stderr[-2000:]}")       # (nothing more runs on the GPU after a failed arm)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit (required: the A/B is against the parent)")
    ap.add_argument("--decodes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=WORKLOADS)
    ap.add_argument("--out")
    ap.add_argument("--arm", nargs=3, metavar=("ROOT", "WORKLOAD", "VARIANTS"), help=argparse.SUPPRESS)
    ap.add_argument("--fingerprint", metavar="ROOT", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.arm:
        return arm(a.arm[0], a.arm[1], a.arm[2].split(","), a.decodes, a.warmup)
    if a.fingerprint:
        return fingerprint_cost(a.fingerprint)
    if not a.parent or not os.path.isdir(a.parent):
        ap.error("--parent DIR (a built checkout of the parent commit) is required")
    if a.reps < 3 or a.decodes < 20:
        ap.error("--reps must be at least 3 and --decodes at least 20")
    lines, md5 = [], {}
    common = ["--decodes", str(a.decodes), "--warmup", str(a.warmup)]
    for wl in a.workloads:
        runs = {"parent": [], "off": [], "cached": [], "verified": []}
        for rep in range(a.reps):
            print(f"{wl}, run {rep + 1}", file=sys.stderr, flush=True)
            r = child(["--arm", os.path.abspath(a.parent), wl, "parent"] + common)
            runs["parent"].append(statistics.median(r["ms"]["parent"]))
            md5["parent"] = r["md5"]
            r = child(["--arm", HERE, wl, "off,cached,verified"] + common)
            md5["this commit"] = r["md5"]
            for v in ("off", "cached", "verified"):
                runs[v].append(statistics.median(r["ms"][v]))
        lines.append(f"{wl}: ms per call, median of {a.decodes} timed calls per variant after {a.warmup} warm-up calls each; {a.reps} runs; "
                     "off / cached / verified alternate inside one process, the parent is a process of its own")
        fig = {v: statistics.median(ms) for v, ms in runs.items()}
        for v, ms in runs.items():
            lines.append(f"  {v:9s} {fig[v]:9.3f}   runs {' '.join(f'{m:.3f}' for m in ms)}")
        lines.append(f"  spread of the parent's runs {max(runs['parent']) - min(runs['parent']):.3f} ms;  off - parent = {fig['off'] - fig['parent']:+.3f} ms;  "
                     f"cached - off = {fig['cached'] - fig['off']:+.3f} ms;  verified - cached = {fig['verified'] - fig['cached']:+.3f} ms")
        lines.append("")
        print("\n".join(lines[-7:]), file=sys.stderr, flush=True)
    f = child(["--fingerprint", HERE])
    lines.append(f"arena of {f['n']} fp32 parameters, us per launch (device events, median of 50): " + ", ".join(f"{k} {v}" for k, v in f["us"].items()))
    lines.append(f"host: model._packs_key() over {f['n_par']} parameters, us per call (mean of 2000): {f['key_us']}")
    lines.append("libortk.so md5: " + ", ".join(f"{k} {v}" for k, v in md5.items()))
    lines.append("")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        notes = ""
        if os.path.exists(a.out):
            old = open(a.out).read().splitlines(keepends=True)
            at = [i for i, l in enumerate(old) if l.startswith(NOTES_MARK)]
            notes = "".join(old[at[0]:]) if at else ""
        with open(a.out, "w") as fh:
            fh.write(text + ("\n" + notes if notes else ""))


if __name__ == "__main__":
    main()
