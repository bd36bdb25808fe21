"""Decoders of the sparse weight images (include/ortk.h: ortk_sparse_plan) back to dense matrices, with the invariants of each format
asserted on the way: shared by tests/test_gpu_ops.py and tests/test_gpu_spmm_exact.py."""
import numpy as np


def ell_slot(k):
    return (k & ~7) | ((k + (k >> 3)) & 7)


def ell_to_dense(plan, bi):
    """Decode block `bi` of a built plan back to a dense (N, K) fp32 matrix (inverse of the device builder)."""
    blk = plan.blocks[bi]
    N, K = blk["N"], blk["K"]
    c0, nch = plan._host[bi].chunk0, (N + 63) // 64
    cp, cl = plan.chunk_ptr.cpu().numpy(), plan.chunk_len.cpu().numpy()
    perm = plan.perm.cpu().numpy()
    st = plan.stream.cpu().numpy().view(np.uint32)
    inv = {ell_slot(k): k for k in range(((K + 7) // 8) * 8)}
    W = np.zeros((N, K), np.float32)
    seen = set()
    for c in range(nch):
        ln, base = int(cl[c0 + c]), int(cp[c0 + c])
        assert ln % (8 if plan.format == 1 else 4) == 0 and base % 2 == 0
        for lane in range(64):
            col = int(perm[(c0 + c) * 64 + lane])
            if col < 0:
                continue
            assert col not in seen and c * 64 // 512 == col // 512          # every column once, inside its 512-column range
            seen.add(col)
            for j in range(ln):
                if plan.format == 1:      # ELL16 pairs: uint2 {off(even) | off(odd) << 16, bf16 w(even) | w(odd) << 16}
                    at = 2 * (base // 2 + (j // 2) * 64 + lane)
                    sh = 16 * (j & 1)
                    off = (int(st[at]) >> sh) & 0xFFFF
                    val = np.array([((int(st[at + 1]) >> sh) & 0xFFFF) << 16], np.uint32).view(np.float32)[0]
                else:
                    off = int(st[2 * (base + j * 64 + lane)])
                    val = st[2 * (base + j * 64 + lane) + 1:2 * (base + j * 64 + lane) + 2].view(np.float32)[0]
                if val != 0:
                    assert off % 16 == 0 and W[col, inv[off // 16]] == 0
                    W[col, inv[off // 16]] = val
    assert seen == set(range(N))
    return W


def gu_to_dense(plan, bi):
    """Decode block `bi` of a built GU16 plan back to a dense (N, K) matrix, checking the invariants of the format: the 4
    address lanes of an entry agree, entries obey the residue rule that makes the LDS gathers conflict-free, every
    non-zero appears exactly once, dummies carry zero weights."""
    blk = plan.blocks[bi]
    N, K = blk["N"], blk["K"]
    slot0, G, nkc = plan._host[bi].chunk0, (N + 15) // 16, (K + 511) // 512
    wf = plan.stream.float().cpu().numpy().reshape(-1, 16, 64, 8)
    ko = plan.chunk_ptr.cpu().numpy().view(np.uint32).reshape(-1, 16, 64)
    ns = plan.chunk_len.cpu().numpy()
    W = np.zeros((((N + 15) // 16) * 16, K), np.float32)
    for g in range(G):
        for kc in range(nkc):
            slot = slot0 + g * nkc + kc
            S = int(ns[slot])
            assert 0 <= S <= 16
            for s in range(S):
                for lg in range(4):
                    for j in range(8):
                        ks = {(int(ko[slot, s, lg * 16 + 4 * (j & 3) + p]) >> (16 * (j >> 2))) & 0xFFFF for p in range(4)}
                        assert len(ks) == 1
                        krel = ks.pop()
                        e = 8 * lg + j
                        assert krel % 8 == ((e & 7) + 4 * ((e >> 3) & 1)) & 7 and krel < 512
                        col = wf[slot, s, lg * 16:(lg + 1) * 16, j]
                        if np.any(col != 0):
                            k = kc * 512 + krel
                            assert k < K and not np.any(W[16 * g:16 * g + 16, k] != 0)
                            W[16 * g:16 * g + 16, k] = col
    assert not np.any(W[N:] != 0)
    return W[:N]
