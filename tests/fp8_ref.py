"""CPU reference of the FP8 weight quantiser (include/ortk.h: ortk_fp8_rows) and the inputs that exercise its edges.

The reference is torch on the CPU: the bf16 weights as fp32, an exact power-of-two scaling, ``.to(torch.float8_e4m3fn)`` (round to
nearest even).  The scaling runs in fp64, where every product of a bf16 value and a power of two in range is exact."""
import torch

BLOCK = 512
E4M3_MAX = 448.0


def fp8_rows_ref(w16):
    """w16: (rows, n_cols) bf16, n_cols a multiple of 512 -> (bytes uint8 (rows, n_cols), scale fp32 (rows, n_cols / 512),
    dequantised fp32 (rows, n_cols))."""
    rows, n_cols = w16.shape
    assert w16.dtype == torch.bfloat16 and n_cols % BLOCK == 0
    w = w16.float().view(rows, n_cols // BLOCK, BLOCK).double()
    amax = w.abs().amax(-1)
    # amax = m 2^ex with 0.5 <= m < 1, and 448 = 0.875 x 2^9: the smallest e with amax 2^-e <= 448
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.875, ex - 9, ex - 8)
    e = torch.where(amax == 0, torch.zeros_like(e), e).double()
    x = (w * torch.pow(2.0, -e)[..., None]).float()
    assert float(x.abs().max()) <= E4M3_MAX
    q = x.to(torch.float8_e4m3fn)
    deq = (q.float().double() * torch.pow(2.0, e)[..., None]).float()
    assert torch.equal(deq.double(), q.float().double() * torch.pow(2.0, e)[..., None])       # representable: nothing rounded
    return q.view(torch.uint8).reshape(rows, n_cols), torch.pow(2.0, e).float(), deq.reshape(rows, n_cols)


def edge_weights(seed=5):
    """(67, 1024) bf16 weights that contain every class of group and value the contract names; returns (weights, {class: (row, block)})."""
    g = torch.Generator().manual_seed(seed)
    rows, n_cols = 67, 1024
    w = torch.zeros(rows, n_cols)
    where = {}
    # rows 0-39: normal rows at magnitudes from 1e-6 to 1e4
    for r in range(40):
        w[r] = torch.randn(n_cols, generator=g) * 10.0 ** (-6 + 10 * r / 39)
    where["all_zero"] = (40, 0)
    w[40, BLOCK:] = torch.randn(BLOCK, generator=g)
    where["one_nonzero"] = (41, 1)
    w[41, :BLOCK] = torch.randn(BLOCK, generator=g) * 0.03
    w[41, BLOCK + 77] = -0.37
    where["negative_zero"] = (42, 0)
    w[42] = torch.randn(n_cols, generator=g)
    w[42, 3:200:7] = -0.0
    # amax exactly 448 x 2^k (e = k), and one bf16 ulp above it: 450 x 2^k (e = k + 1)
    for i, k in enumerate((3, -5, 0, -20)):
        for j, top in enumerate((448.0, 450.0)):
            r, b = 43 + i, j
            w[r, b * BLOCK:(b + 1) * BLOCK] = (torch.rand(BLOCK, generator=g) * 2 - 1) * 400.0 * 2.0 ** k
            w[r, b * BLOCK + 11 * (i + 1)] = (top if (i + j) % 2 == 0 else -top) * 2.0 ** k
            where[f"amax_{'448' if j == 0 else 'ulp_above'}_k{k}"] = (r, b, k + j)
    # amax 448 (e = 0) and values exactly halfway between e4m3 neighbours, both parities, both signs, every binade
    ties = [(1 + (m + 0.5) / 8) * 2.0 ** ex for ex in range(-6, 9) for m in range(8) if (1 + (m + 0.5) / 8) * 2.0 ** ex < E4M3_MAX]
    where["ties"] = (47, 0)
    w[47, 0] = E4M3_MAX
    w[47, 1:1 + len(ties)] = torch.tensor(ties)
    w[47, 200:200 + len(ties)] = -torch.tensor(ties)
    # the same under a scale: a group whose e is -7
    where["ties_scaled"] = (47, 1)
    w[47, BLOCK] = -E4M3_MAX * 2.0 ** -7
    w[47, BLOCK + 1:BLOCK + 1 + len(ties)] = torch.tensor(ties) * 2.0 ** -7
    # e4m3's subnormal range (multiples of 2^-9 below 2^-6), the ties between them (odd multiples of 2^-10), and values at and below
    # half the smallest subnormal (2^-10: a tie that goes to zero; 2^-11, 3 x 2^-12, 2^-20: zero; 5 x 2^-12: 2^-9), both signs
    sub = [k * 2.0 ** -10 for k in range(1, 33)] + [2.0 ** -11, 3 * 2.0 ** -12, 2.0 ** -20, 5 * 2.0 ** -12, 2.0 ** -40]
    where["subnormal"] = (48, 0)
    w[48, 0] = E4M3_MAX
    w[48, 1:1 + len(sub)] = torch.tensor(sub)
    w[48, 100:100 + len(sub)] = -torch.tensor(sub)
    where["subnormal_scaled"] = (48, 1)
    w[48, BLOCK] = E4M3_MAX * 2.0 ** 5
    w[48, BLOCK + 1:BLOCK + 1 + len(sub)] = torch.tensor(sub) * 2.0 ** 5
    # rows 49-66: normal rows again, one magnitude per block
    for r in range(49, rows):
        w[r, :BLOCK] = torch.randn(BLOCK, generator=g) * 10.0 ** (-6 + 10 * (r - 49) / 17)
        w[r, BLOCK:] = torch.randn(BLOCK, generator=g) * 10.0 ** (4 - 10 * (r - 49) / 17)
    w16 = w.bfloat16()
    assert torch.equal(w16[47].float(), w[47]) and torch.equal(w16[48].float(), w[48])
    for name, at in where.items():
        if name.startswith("amax_"):
            r, b, e = at
            top = (448.0 if "448" in name else 450.0) * 2.0 ** (e - (0 if "448" in name else 1))
            assert float(w16[r, b * BLOCK:(b + 1) * BLOCK].float().abs().max()) == top, name
    return w16, where
