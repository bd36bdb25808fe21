"""ortk_layernorm_bwd at the model width (512), as the XE step calls it (bf16 output gradient, residual gradient in, masked bf16 copy
out, dropout 0.1), at the step's three row counts: the atomics form (ortk_layernorm_bwd_dt) against the partials form
(ortk_layernorm_bwd_part), interleaved in one process, three rounds; then ortk_ln_partials_reduce alone for the 19 slots of the decoder
half and the 13 of the encoder half.

  python scratch/ln_bench.py [LIB ...]

Every LIB is another libortk.so whose ortk_norm.hip was compiled with -DORTK_LN_PART_ROWS=r -DORTK_LN_PART_MAX_BLOCKS=c (the rows-per-block
sweep): its partials form is timed in the same rounds.  --forms adds the older comparison (four / eight columns per lane, fp32 dy)."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import sparse_image_captioning_amd as P
L = P._lib; lib = L.lib()
forms = "--forms" in sys.argv
libs = [("this build", lib)]
for path in (a for a in sys.argv[1:] if not a.startswith("--")):
    h = C.CDLL(path)
    for name in ("ortk_layernorm_bwd_part", "ortk_ln_part_blocks", "ortk_ln_part_rows"):
        getattr(h, name).restype, getattr(h, name).argtypes = L.SIGNATURES[name]
    libs.append((os.path.basename(path), h))
d, BYTES_PER_ROW = 512, 8 * 1024
def timeit(f, n=30):
    for _ in range(3): f()
    torch.cuda.synchronize(); e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n
for rows in (16640, 21760, 9216):
    x = torch.randn(rows, d, device="cuda"); dy = torch.randn(rows, d, device="cuda"); a = torch.randn(d, device="cuda"); b = torch.randn(d, device="cuda")
    dy16 = dy.bfloat16()
    y = torch.empty(rows, d, device="cuda"); st = torch.empty(rows, 2, device="cuda"); dres = torch.randn(rows, d, device="cuda")
    dx = torch.empty_like(x); da = torch.zeros(d, device="cuda"); db = torch.zeros(d, device="cuda"); dz = torch.empty(rows, d, device="cuda", dtype=torch.bfloat16)
    part = torch.empty(1024, 2, d, device="cuda"); nb = C.c_int32(0)
    L.check(lib.ortk_layernorm_fwd(L.ptr(x), L.ptr(a), L.ptr(b), L.ptr(y), 0, L.ptr(st), rows, d, 1e-6, L.stream_ptr()), "f")
    def run(g, dt):
        return lambda: lib.ortk_layernorm_bwd_dt(L.ptr(g), dt, L.ptr(x), L.ptr(a), L.ptr(st), L.ptr(dres), L.ptr(dx), L.ptr(da), L.ptr(db), rows, d, 1e-6,
                                                 L.ptr(dz), 1, 0.1, 7, None, L.stream_ptr())
    def run_part(h):
        return lambda: h.ortk_layernorm_bwd_part(L.ptr(dy16), 1, L.ptr(x), L.ptr(a), L.ptr(st), L.ptr(dres), L.ptr(dx), L.ptr(part), 1024, C.byref(nb), rows, d, 1e-6,
                                                 L.ptr(dz), 1, 0.1, 7, None, L.stream_ptr())
    if forms:
        L.set_tuning(ln_fuse=4); t4 = timeit(run(dy, 0)); dx4 = dx.clone()
        L.set_tuning(ln_fuse=0); t8 = timeit(run(dy, 0))
        assert (dx - dx4).abs().max().item() <= 2e-6 * dx4.abs().max().item(), "eight-column form != four-column form"      # (the row sums add in another order)
        print(f"rows {rows}: fp32 dy, four columns {t4:.1f} us | eight columns {t8:.1f} us", flush=True)
    # the two forms give the same dx / dz, and the partials add up to the atomics' da / db
    da.zero_(); db.zero_(); L.check(run(dy16, 1)(), "atomics"); dxa, dza, daa, dba = dx.clone(), dz.clone(), da.clone(), db.clone()
    dx.zero_(); dz.zero_(); da.zero_(); db.zero_(); L.check(run_part(lib)(), "partials")
    slot = L.LnSlot(part.data_ptr(), nb.value, da.data_ptr(), db.data_ptr())
    L.check(lib.ortk_ln_partials_reduce(C.byref(slot), 1, L.stream_ptr()), "reduce")
    assert torch.equal(dx, dxa) and torch.equal(dz, dza)
    err = max(((da - daa).abs().max() / daa.abs().max()).item(), ((db - dba).abs().max() / dba.abs().max()).item())
    assert err < 1e-5, err
    floor = rows * BYTES_PER_ROW / 6.0e6       # us at 6.0 TB/s (profiles/r03_fetch_rate_probe.txt)
    res = {"atomics": []}
    for _ in range(3):
        res["atomics"].append(timeit(run(dy16, 1)))
        for name, h in libs:
            t = timeit(run_part(h))
            res.setdefault(f"partials, {name}: {h.ortk_ln_part_rows()} rows per block, {nb.value} blocks", []).append(t)
    print(f"rows {rows} (bytes / 6.0 TB/s = {floor:.1f} us)", flush=True)
    for k, v in res.items():
        print(f"  {k}: " + " ".join(f"{t:.1f}" for t in v) + f" us  (mean {sum(v) / 3:.1f}, {sum(v) / 3 - floor:+.1f} to the floor)", flush=True)
# the reduce launch alone: the decoder half's 19 slots (16 640 rows each) and the encoder half's 13 (9 216 rows each)
for n, rows in ((19, 16640), (13, 9216)):
    blocks = lib.ortk_ln_part_blocks(rows)
    parts = torch.randn(n, blocks, 2, d, device="cuda"); dst = torch.zeros(n, 2, d, device="cuda")
    slots = (L.LnSlot * n)(*[L.LnSlot(parts[i].data_ptr(), blocks, dst[i, 0].data_ptr(), dst[i, 1].data_ptr()) for i in range(n)])
    L.check(lib.ortk_ln_partials_reduce(slots, n, L.stream_ptr()), "reduce")
    ref = parts.double().sum(1)
    assert ((dst - ref).abs().max() / ref.abs().max()).item() < 1e-5
    ts = [timeit(lambda: lib.ortk_ln_partials_reduce(slots, n, L.stream_ptr())) for _ in range(3)]
    print(f"reduce alone, {n} slots x {blocks} blocks ({n * blocks * 4096 / 1e6:.1f} MB): " + " ".join(f"{t:.1f}" for t in ts) + " us", flush=True)
