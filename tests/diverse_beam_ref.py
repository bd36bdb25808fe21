"""CPU restatement of the diverse beam search (group_size > 1) for the diverse-beam tests, on the oracle's `encode` /
`DecodeState` / `decode_step` as tests/beam_ref.py is.

What it restates is CaptionModel.batch_beam_search (models/caption_model.py:33-52, 151-218) with two repairs: the
undefined `repeat_tensor` is the row-wise repeat of the file's upstream, and every group is embedded at ITS OWN position (the
reference's PositionalEncoding counts module calls, so the groups, which take turns inside one time loop, drift apart).

  * b beams in G groups of bd = b / G; every group is a beam search of width bd with its own histories, cumulative scores,
    caches (one DecodeState per group) and finished list; the BOS pass is shared.
  * staggered schedule: global step T = 0 .. L + G - 2, inside it g = 0 .. G - 1, group g does its local step t = T - g.
  * in that step the log-probs lose fl32(cnt * lambda), cnt[n, v] = how many current beams of groups 0 .. g-1 of image n hold v at
    column t of their histories as they stand NOW (those groups are ahead and have re-ordered their histories since).
  * the stored token log-prob is the unaugmented one, cum the augmented sum.

Per image, `min_gap` is the smallest difference between consecutive entries among the best bd + 1 candidates of any step of any
group, and among the best bd + 1 finished scores of any group: an image below GAP holds a pair the fp32 parity mode is not
required to order."""
import numpy as np
import torch
import torch.nn.functional as F

import beam_ref as R
from oracle import ort_oracle as O

GAP = R.GAP
N_IMG = R.N_IMG

# case -> (b, G, decode options, first input seed tried, images that must have min_gap >= GAP)
CASES = {
    "b4_g2": (4, 2, {}, 75, 4),
    "b6_g3_l08_t09": (6, 3, {"diversity_lambda": 0.8, "temperature": 0.9}, 75, 4),
    "b4_g4": (4, 4, {}, 75, 4),
    "b6_g2_l0": (6, 2, {"diversity_lambda": 0.0}, 75, 4),
    "b8_g2_wu_dc": (8, 2, {"length_penalty": "wu_0.7", "decoding_constraint": 1}, 75, 4),
    "b32_g4_l03": (32, 4, {"diversity_lambda": 0.3}, 75, 2),
}


def _fork(st):
    """an independent DecodeState with the same caches (the tensors are never written in place)"""
    n = O.DecodeState(st.P, st.cfg, st.memory, st.att_masks)
    n.step = st.step
    n.self_k, n.self_v, n.src_k, n.src_v = list(st.self_k), list(st.self_v), list(st.src_k), list(st.src_v)
    return n


def diverse_beam_search(P, cfg, att_feats, boxes, att_masks, beam_size, group_size, diversity_lambda=0.5, temperature=1.0,
                        decoding_constraint=0, length_penalty=""):
    """seq (N, b, L), seq_logprobs (N, b, L), p (N, b) with group g in rows g * bd .. (g + 1) * bd - 1, and min_gap (N,) float64."""
    L, V, b, G = cfg.max_seq_length, cfg.vocab_size, int(beam_size), int(group_size)
    assert 1 <= G <= b and b % G == 0
    bd = b // G
    lam = torch.tensor(float(np.float32(diversity_lambda)), dtype=torch.float32)
    pen = O._length_penalty(length_penalty)
    mem = O.encode(P, cfg, att_feats, boxes, att_masks)
    N = att_feats.size(0)
    st0 = O.DecodeState(P, cfg, mem, att_masks)
    logp0 = O.decode_step(st0, torch.full((N,), cfg.bos_token_id, dtype=torch.long))
    sts, logps = [], []
    for g in range(G):
        s = _fork(st0)
        s.repeat(bd)
        sts.append(s)
        logps.append(logp0)
    seqs = [torch.zeros(N, bd, 0, dtype=torch.long) for _ in range(G)]
    tok_lps = [torch.zeros(N, bd, 0) for _ in range(G)]
    cums = [torch.zeros(N, bd) for _ in range(G)]
    done = [[[] for _ in range(G)] for _ in range(N)]
    min_gap = torch.full((N,), float("inf"), dtype=torch.float64)
    for T in range(L + G - 1):
        for g in range(G):
            t = T - g
            if t < 0 or t > L - 1:
                continue
            logp = logps[g]
            if decoding_constraint and t > 0:
                logp = logp.scatter(1, seqs[g][:, :, t - 1].reshape(-1, 1), float("-inf"))
            unaug = logp
            if g > 0:
                cnt = torch.zeros(N, V)
                for p_ in range(g):
                    cnt.scatter_add_(1, seqs[p_][:, :, t], torch.ones(N, bd))
                change = cnt * lam                                              # one fp32 multiply
                logp = logp - (change if t == 0 else change.repeat_interleave(bd, 0))      # one fp32 subtract
            lp3 = logp.reshape(N, -1, V)
            cand = (cums[g][:, :1] if t == 0 else cums[g]).unsqueeze(-1) + lp3
            ys, ix = torch.sort(cand.reshape(N, -1), -1, True)
            min_gap = torch.minimum(min_gap, R._gaps(ys, bd))
            ys, ix = ys[:, :bd], ix[:, :bd]
            parent = ix // V
            tok = ix % V
            if t > 0:
                seqs[g] = seqs[g].gather(1, parent[:, :, None].expand_as(seqs[g]))
                tok_lps[g] = tok_lps[g].gather(1, parent[:, :, None].expand_as(tok_lps[g]))
            seqs[g] = torch.cat([seqs[g], tok[:, :, None]], -1)
            tok_lps[g] = torch.cat([tok_lps[g], unaug.reshape(N, -1).gather(1, ix)[:, :, None]], -1)
            cum = ys.clone()
            if t > 0:
                sts[g].reorder((parent + torch.arange(N)[:, None] * bd).reshape(-1))
            is_end = tok == cfg.eos_token_id
            if t == L - 1:
                is_end = torch.ones_like(is_end)
            for n in range(N):
                for q in range(bd):
                    if is_end[n, q]:
                        done[n][g].append(dict(seq=seqs[g][n, q].clone(), lps=tok_lps[g][n, q].clone(), p=pen(t + 1, cum[n, q].item())))
            cums[g] = cum - 1000.0 * is_end.float()
            if t < L - 1:
                nxt = O.decode_step(sts[g], tok.reshape(-1))
                logps[g] = F.log_softmax(nxt / temperature, dim=-1)
    seq = torch.zeros(N, b, L, dtype=torch.long)
    seq_lp = torch.zeros(N, b, L)
    ps = torch.zeros(N, b)
    for n in range(N):
        for g in range(G):
            ranked = sorted(done[n][g], key=lambda d: -d["p"])
            fin = torch.tensor([[d["p"] for d in ranked]], dtype=torch.float64)
            min_gap[n] = min(float(min_gap[n]), float(R._gaps(fin, bd)[0]))
            for q, d in enumerate(ranked[:bd]):
                ln = d["seq"].numel()
                seq[n, g * bd + q, :ln] = d["seq"]
                seq_lp[n, g * bd + q, :ln] = d["lps"]
                ps[n, g * bd + q] = d["p"]
    return seq, seq_lp, ps, min_gap


case_inputs = R.case_inputs
