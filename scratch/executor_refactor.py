"""Two builds of the executor side by side (profiles/executor_refactor.txt): the schedule as two sequences, and the outputs of bench.py.

    rocprofv3 --hip-trace --kernel-trace --output-format csv -d DIR -- python scratch/executor_refactor.py step side_stream=0
    python scratch/executor_refactor.py digest DIR OUT      # OUT.api: HIP API call names in call order
                                                            # OUT.kernels: kernel, grid, workgroup, LDS, queue in dispatch order
    python scratch/executor_refactor.py compare OUT_A OUT_B
    python scratch/executor_refactor.py results A1 A2 B      # bench.py --dump-outputs directories: two runs of build A, one of build B;
                                                            # every array A reproduces bit for bit must be bit-equal in B

`step` runs four XE steps of the benchmark's geometry (256 images x 5 captions, bf16) under the ortk_tuning switches given as k=v;
`digest` also takes the trace of a bench.py run.  Queues are numbered in order of first appearance: the handles differ from process to
process."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def step(switches):
    sys.path.insert(0, ROOT)
    import torch
    import bench as Bn
    import sparse_image_captioning_amd as pkg
    from sparse_image_captioning_amd.utils.config import ort_config
    from sparse_image_captioning_amd.training import NativeTrainer
    dev = torch.device("cuda", 0)
    cfg = ort_config(drop_prob_src=0.5, max_seq_length=18)
    pkg._lib.set_tuning(**{k: int(v) for k, v in (s.split("=") for s in switches)})
    torch.manual_seed(8888)
    m = pkg.get_model("relation_transformer")(cfg, precision="bf16").to(dev).train()
    b = Bn.synth_batch(256, 36, cfg.att_feat_size, cfg.vocab_size, 5, cfg.max_seq_length, 1000, dev)
    tr = NativeTrainer(m, noamopt_factor=1.0, noamopt_warmup=20000)
    for _ in range(4):
        loss = tr.xe_step(b)
    torch.cuda.synchronize()
    print("loss", float(loss))


def _rows(d, kind):
    files = glob.glob(os.path.join(d, "**", f"*{kind}.csv"), recursive=True)
    assert len(files) == 1, (kind, files)
    with open(files[0], newline="") as f:
        return list(csv.DictReader(f))


def digest(d, out):
    api = sorted(_rows(d, "hip_api_trace"), key=lambda r: int(r["Start_Timestamp"]))
    with open(out + ".api", "w") as f:
        f.writelines(r["Function"] + "\n" for r in api)
    ker = sorted(_rows(d, "kernel_trace"), key=lambda r: int(r["Dispatch_Id"]))
    queues = {}
    with open(out + ".kernels", "w") as f:
        for r in ker:
            q = queues.setdefault(r["Queue_Id"], len(queues))
            grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
            wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
            lds = r["LDS_Block_Size"] if "LDS_Block_Size" in r else r["Group_Segment_Size"]      # (the column's name in older rocprofv3)
            f.write(f'{r["Kernel_Name"]} grid={grid} wg={wg} lds={lds} queue={q}\n')
    print(f"{out}: {len(api)} HIP API calls, {len(ker)} dispatches on {len(queues)} queues")


def compare(a, b):
    ok = True
    for ext in (".api", ".kernels"):
        x, y = open(a + ext).read().splitlines(), open(b + ext).read().splitlines()
        first = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), None if len(x) == len(y) else min(len(x), len(y)))
        print(f"{os.path.basename(a)}{ext}: {len(x)} vs {len(y)} entries; sequences equal: {first is None}")
        if first is not None:
            ok = False
            print(f"  first difference at {first}:\n    {x[first] if first < len(x) else '<end>'}\n    {y[first] if first < len(y) else '<end>'}")
    return 0 if ok else 1


def results(a1, a2, b):
    import numpy as np
    ok = True
    for f in sorted(os.listdir(a1)):
        x, y, z = (np.load(os.path.join(d, f)) for d in (a1, a2, b))
        diff = lambda p, q: "bit-equal" if p.shape == q.shape and p.tobytes() == q.tobytes() else \
            "%.3e" % float(np.abs(p.astype(np.float64) - q.astype(np.float64)).max()) if p.shape == q.shape else "shape"
        pp, pc = diff(x, y), diff(x, z)
        good = pc == "bit-equal" or (pp != "bit-equal" and pc != "shape")
        ok = ok and good
        print(f"  {f:24s} {str(x.dtype):8s} {str(x.shape):18s} parent-vs-parent  {pp:10s}  parent-vs-child  {pc:10s}  {'ok' if good else 'DIFFERS'}")
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "step":
        step(sys.argv[2:])
    elif sys.argv[1] == "digest":
        digest(sys.argv[2], sys.argv[3])
    elif sys.argv[1] == "results":
        sys.exit(results(*sys.argv[2:5]))
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
