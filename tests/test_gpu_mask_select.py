"""ortk_mask_select (csrc/ortk_select.hip) through the C ABI on plain device tensors: in every group of arena segments the n_drop
smallest criteria get mask 0, the rest 1, and among equal keys at the threshold the LOWEST positions in group order go.

The yardstick is `yardstick()` below — a stable argsort of the uint32 keys in group order with the first n_drop entries dropped:
the tie rule in a few lines.  Blind / uniform results must equal it bit for bit; dist (kind 1) is compared with torch's own
expression under a near-threshold condition (see that test)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 4096        # elements per workgroup: small, so that the 4 097- and 70 001-element segments span chunks with partial tails
EINVAL = -1
RAGGED = (1, 63, 64, 4097, 70001)


@pytest.fixture(scope="module")
def P():
    import sparse_image_captioning_amd as pkg
    pkg._lib.require_gpu()
    return pkg


def keys_of(c):
    """fp32 criterion (>= 0 up to the sign bit) -> monotone uint32 key: -0.0 == +0.0, denormals kept, NaN above +inf."""
    return np.ascontiguousarray(c, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def yardstick(keys, n_drop):
    order = np.argsort(keys, kind="stable")
    mask = np.ones(keys.size, np.float32)
    mask[order[:n_drop]] = 0.0
    return mask


def layout(sizes, guard=128):
    """[(offset, numel)] with every offset a multiple of 64 (as arena entries), a gap after each segment, a guard band at both ends."""
    off, segs = guard, []
    for n in sizes:
        segs.append((off, n))
        off = (off + n + 63) // 64 * 64 + 64
    return segs, off + guard


def arenas(segs, total, values):
    """weights: NaN everywhere outside the segments; mask: 7.0 everywhere (the call must overwrite exactly the segments)."""
    w = torch.full((total,), float("nan"))
    for (o, n), v in zip(segs, values):
        w[o:o + n] = v
    return w.cuda(), torch.full((total,), 7.0).cuda()


def group_index(segs, groups, g):
    return np.concatenate([np.arange(o, o + n) for (o, n), gg in zip(segs, groups) if gg == g])


def expected(crit, mask0, segs, groups, n_drop):
    out = mask0.copy()
    for g, k in enumerate(n_drop):
        idx = group_index(segs, groups, g)
        out[idx] = yardstick(keys_of(crit[idx]), k)
    return out


def select(P, w, mask, segs, groups, n_drop, kind, chunk=CHUNK, override=None):
    """One call; `override(args)` may damage the argument list (the refusal test).  Returns the status after a synchronise."""
    L = P._lib
    dev = mask.device
    chunks = [(i, s, min(chunk, n - s)) for i, (_, n) in enumerate(segs) for s in range(0, n, chunk)]
    i64 = lambda v: torch.tensor(list(v), dtype=torch.int64, device=dev)
    tables = [i64(o for o, _ in segs), i64(n for _, n in segs), i64(groups)] + [i64(col) for col in zip(*chunks)] + [i64(n_drop)]
    counts = [len(segs), len(n_drop), len(chunks), kind]
    ws = torch.full((L.lib().ortk_mask_select_workspace_bytes(*counts),), 255, dtype=torch.uint8, device=dev)   # (not pre-cleared)
    args = dict(w=L.ptr(w), mask=L.ptr(mask), tables=[L.ptr(t) for t in tables], counts=counts, ws=L.ptr(ws), ws_bytes=ws.numel())
    if override:
        override(args)
    rc = L.lib().ortk_mask_select(args["w"], args["mask"], *args["tables"], *args["counts"], args["ws"], args["ws_bytes"], L.stream_ptr())
    torch.cuda.synchronize()
    return rc


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def check_exact(P, w, mask, segs, groups, n_drop, kind=0):
    mask0 = mask.cpu().numpy()
    assert select(P, w, mask, segs, groups, n_drop, kind) == 0
    got = mask.cpu().numpy()
    want = expected(w.cpu().numpy(), mask0, segs, groups, n_drop)
    diff = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert diff.size == 0, (diff.size, diff[:8], got[diff[:8]], want[diff[:8]])
    inside = np.zeros(got.size, bool)
    for o, n in segs:
        inside[o:o + n] = True
    assert np.all(got[~inside] == 7.0), "a position outside the listed segments was written"
    n = int(inside.sum())
    assert float(got[inside].astype(np.float64).sum()) == n - sum(n_drop)
    return got


@pytest.fixture(scope="module")
def ragged():
    torch.manual_seed(1234)
    segs, total = layout(RAGGED)
    return segs, total, [torch.randn(n) for _, n in segs]


@pytest.mark.parametrize("target", [0.0, 0.5, 0.95, "all_but_one"])
def test_ragged_segments_blind(P, ragged, target):
    segs, total, values = ragged
    w, mask = arenas(segs, total, values)
    n = sum(RAGGED)
    n_drop = n - 1 if target == "all_but_one" else int(target * n)
    check_exact(P, w, mask, segs, [0] * len(segs), [n_drop])


def test_ragged_segments_blind_offsets_off_the_16_byte_grid(P, ragged):
    """The same segments at odd arena offsets: every range takes the element-wise path."""
    _, _, values = ragged
    segs, off = [], 129
    for n in RAGGED:
        segs.append((off, n))
        off += n + 67 + (off + n) % 2
    w, mask = arenas(segs, off + 128, values)
    assert all(o % 4 for o, _ in segs[:2])
    check_exact(P, w, mask, segs, [0] * len(segs), [int(0.5 * sum(RAGGED))])


@pytest.mark.parametrize("inside", ["zero", "quarter"])
def test_ties_lowest_positions_go_and_reruns_are_identical(P, inside):
    torch.manual_seed(77)
    segs, total = layout((30000, 10001))
    values = [torch.round(torch.randn(n) * 4) / 4 for _, n in segs]
    zeros = torch.zeros(5000)
    zeros[torch.rand(5000) < 0.5] = -0.0
    values[0][2000:7000] = zeros                                    # spans two chunks of the first segment
    values[1][5:9] = torch.tensor([1e-45, -3e-39, 1.1e-38, -1e-45])  # denormals: ordinary keys between 0 and 0.25
    values[0][11], values[0][12], values[1][0], values[1][1] = float("inf"), float("-inf"), float("-inf"), float("inf")
    w, mask = arenas(segs, total, values)
    keys = keys_of(torch.cat(values).numpy())
    k0, k25 = int((keys == 0).sum()), int((keys == keys_of(np.float32(0.25))[0]).sum())
    assert k0 >= 5000 and k25 > 100 and int(np.signbit(torch.cat(values).numpy()[keys == 0]).sum()) > 1000
    below25 = int((keys < keys_of(np.float32(0.25))[0]).sum())
    assert below25 == k0 + 4
    n_drop = k0 // 2 if inside == "zero" else below25 + k25 // 3
    first = check_exact(P, w, mask, segs, [0, 0], [n_drop])
    again = torch.full_like(mask, 7.0)
    assert select(P, w, again, segs, [0, 0], [n_drop], 0) == 0
    assert same_bits(first, again.cpu().numpy())


@pytest.mark.parametrize("target", [0.3, 0.5, 0.95])
def test_keys_that_differ_in_the_last_byte_only(P, target):
    """w = 1 + k * 2^-23, k in 0..199: the first three radix passes see one digit, the fourth decides, with ~250 ties per key."""
    torch.manual_seed(5)
    n = 50000
    segs, total = layout((n,))
    k = torch.randint(0, 200, (n,))
    v = (1.0 + k.double() * 2.0 ** -23).float()
    assert len(set(keys_of(v.numpy()) >> 8)) == 1 and len(set(keys_of(v.numpy()))) == 200
    w, mask = arenas(segs, total, [v])
    check_exact(P, w, mask, segs, [0], [int(target * n)])


@pytest.mark.parametrize("target", [0.5, 0.95])
def test_uniform_one_group_per_segment(P, ragged, target):
    segs, total, values = ragged
    w, mask = arenas(segs, total, values)
    n_drop = [int(target * n) for n in RAGGED]
    assert n_drop[0] == 0
    check_exact(P, w, mask, segs, list(range(len(segs))), n_drop)


def test_dist_against_torch_expression(P):
    """Kind 1 against torch's `((w - w.mean()) / w.std(unbiased=False)).abs()` evaluated on the device.  torch sums mean and std in
    fp32 in its own order, the kernel in fp64 and rounds: mean or std can differ by an fp32 ulp, which moves c by ~1e-7 relative.
    So the two masks may differ, but only at positions whose torch criterion lies within a relative 1e-5 of the threshold value; the
    0.1 % cap on their number is a guard (checked on the CPU with numpy for this seed: moving every non-constant segment's mean and
    std by one fp32 ulp, in all nine combinations of directions, changes none of the 25 494 positions)."""
    torch.manual_seed(2024)
    sizes = (1000, 4097, 20000, 333, 64)
    segs, total = layout(sizes)
    values = [torch.randn(1000) * 0.02 + 0.001, torch.randn(4097) * 0.5 - 0.3, torch.randn(20000) * 0.1, torch.randn(333) * 3.0 + 10.0,
              torch.full((64,), 0.25)]
    w, mask = arenas(segs, total, values)
    n = sum(sizes)
    n_drop = int(0.8 * n)
    crit = torch.full_like(w, float("nan"))
    for o, m in segs:
        x = w[o:o + m]
        crit[o:o + m] = ((x - x.mean()) / x.std(unbiased=False)).abs()
    crit = crit.cpu().numpy()
    groups = [0] * len(segs)
    mask0 = mask.cpu().numpy()
    assert select(P, w, mask, segs, groups, [n_drop], 1) == 0
    got, want = mask.cpu().numpy(), expected(crit, mask0, segs, groups, [n_drop])
    idx = group_index(segs, groups, 0)
    assert np.all(np.delete(got, idx) == 7.0)
    assert set(np.unique(got[idx])) <= {0.0, 1.0}
    assert float(got[idx].astype(np.float64).sum()) == n - n_drop
    o, m = segs[-1]
    assert np.all(np.isnan(crit[o:o + m])) and np.all(got[o:o + m] == 1.0), "the constant segment is 0/0 = NaN: dropped last"
    threshold = np.sort(crit[idx])[n_drop - 1]
    diff = idx[got[idx] != want[idx]]
    print("dist: positions that differ from torch's criterion:", diff.size, "threshold", threshold)
    assert np.all(np.abs(crit[diff] - threshold) <= 1e-5 * threshold), (crit[diff], threshold)
    assert diff.size <= 1e-3 * n, diff.size
    again = torch.full_like(mask, 7.0)
    assert select(P, w, again, segs, groups, [n_drop], 1) == 0
    assert same_bits(got, again.cpu().numpy())


@pytest.mark.parametrize("what", ["null_weights", "null_table", "zero_segments", "kind_9", "one_byte_workspace", "too_many_segments"])
def test_refusals_leave_the_mask_alone(P, ragged, what):
    segs, total, values = ragged
    w, mask = arenas(segs, total, values)

    def damage(a):
        if what == "null_weights":
            a["w"] = None
        elif what == "null_table":
            a["tables"][4] = None
        elif what == "zero_segments":
            a["counts"][0] = 0
        elif what == "kind_9":
            a["counts"][3] = 9
        elif what == "one_byte_workspace":
            a["ws_bytes"] = 1
        elif what == "too_many_segments":
            a["counts"][0] = 4097
    assert select(P, w, mask, segs, [0] * len(segs), [100], 0, override=damage) == EINVAL
    assert np.all(mask.cpu().numpy() == 7.0)
    assert P._lib.lib().ortk_mask_select_workspace_bytes(0, 1, 1, 0) == 0 and P._lib.lib().ortk_mask_select_workspace_bytes(1, 1, 1, 9) == 0
