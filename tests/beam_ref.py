"""CPU restatement of the beam loop for the wide-beam tests: what `oracle.beam_search` computes (same operations on the same
tensors, so the results are bit-identical), plus, per image, `min_gap` — the smallest difference between consecutive entries
among the best b + 1 candidates of any step and among the best b + 1 finished scores after the length penalty.  An image whose
min_gap is below GAP holds a pair the fp32 parity mode is not required to order; the exact comparisons leave it out."""
import torch
import torch.nn.functional as F

from oracle import ort_oracle as O

# the bar the golden tests grant the parity mode's token log-probs and beam scores (close(.., 2e-4)); 18 x the 1.1e-5 by which the
# reference and the oracle differ on a CPU
GAP = 2e-4

# case -> (width, decode options, input seed, images that must have min_gap >= GAP)
CASES = {
    "b10": (10, {}, 75, 4),
    "b12_wu_dc": (12, {"length_penalty": "wu_0.7", "decoding_constraint": 1}, 75, 4),
    "b16": (16, {}, 75, 4),
    "b32": (32, {}, 69, 2),
}
N_IMG = 4


def _gaps(sorted_desc, b):
    """smallest difference of consecutive entries among the first b + 1 of a descending (N, n) tensor -> (N,)"""
    top = sorted_desc[:, :b + 1].double()
    if top.size(1) < 2:
        return torch.full((top.size(0),), float("inf"), dtype=torch.float64)
    return (top[:, :-1] - top[:, 1:]).min(1).values


def beam_search(P, cfg, att_feats, boxes, att_masks, beam_size, temperature=1.0, decoding_constraint=0, length_penalty=""):
    """seq (N, b, L), seq_logprobs (N, b, L), p (N, b) as `oracle.beam_search`, and min_gap (N,) float64."""
    L, V, b = cfg.max_seq_length, cfg.vocab_size, beam_size
    pen = O._length_penalty(length_penalty)
    mem = O.encode(P, cfg, att_feats, boxes, att_masks)
    N = att_feats.size(0)
    st = O.DecodeState(P, cfg, mem, att_masks)
    logp = O.decode_step(st, torch.full((N,), cfg.bos_token_id, dtype=torch.long))
    st.repeat(b)
    beam_seq = torch.zeros(N, b, 0, dtype=torch.long)
    beam_tok_lp = torch.zeros(N, b, 0)
    cum = torch.zeros(N, b)
    done = [[] for _ in range(N)]
    min_gap = torch.full((N,), float("inf"), dtype=torch.float64)
    for t in range(L):
        if decoding_constraint and t > 0:
            logp = logp.scatter(1, beam_seq[:, :, t - 1].reshape(-1, 1), float("-inf"))
        lp3 = logp.reshape(N, -1, V)
        cand = (cum[:, :1] if t == 0 else cum).unsqueeze(-1) + lp3
        ys, ix = torch.sort(cand.reshape(N, -1), -1, True)
        min_gap = torch.minimum(min_gap, _gaps(ys, b))
        ys, ix = ys[:, :b], ix[:, :b]
        parent = ix // V
        tok = ix % V
        if t > 0:
            beam_seq = beam_seq.gather(1, parent[:, :, None].expand_as(beam_seq))
            beam_tok_lp = beam_tok_lp.gather(1, parent[:, :, None].expand_as(beam_tok_lp))
        beam_seq = torch.cat([beam_seq, tok[:, :, None]], -1)
        beam_tok_lp = torch.cat([beam_tok_lp, lp3.reshape(N, -1).gather(1, ix)[:, :, None]], -1)
        cum = ys.clone()
        state_ix = (parent + torch.arange(N)[:, None] * lp3.size(1)).reshape(-1)
        if t > 0:
            st.reorder(state_ix)
        is_end = tok == cfg.eos_token_id
        if t == L - 1:
            is_end = torch.ones_like(is_end)
        for n in range(N):
            for q in range(b):
                if is_end[n, q]:
                    done[n].append(dict(seq=beam_seq[n, q].clone(), lps=beam_tok_lp[n, q].clone(), p=pen(t + 1, cum[n, q].item())))
        cum = cum - 1000.0 * is_end.float()
        if t < L - 1:
            logp = O.decode_step(st, tok.reshape(-1))
            logp = F.log_softmax(logp / temperature, dim=-1)
    seq = torch.zeros(N, b, L, dtype=torch.long)
    seq_lp = torch.zeros(N, b, L)
    ps = torch.zeros(N, b)
    for n in range(N):
        ranked = sorted(done[n], key=lambda d: -d["p"])
        fin = torch.tensor([[d["p"] for d in ranked]], dtype=torch.float64)
        min_gap[n] = min(float(min_gap[n]), float(_gaps(fin, b)[0]))
        for q, d in enumerate(ranked[:b]):
            ln = d["seq"].numel()
            seq[n, q, :ln] = d["seq"]
            seq_lp[n, q, :ln] = d["lps"]
            ps[n, q] = d["p"]
    return seq, seq_lp, ps, min_gap


def case_inputs(C, seed):
    """the G1 input recipe with N_IMG images and the case's seed (tests/golden/common.py: make_inputs)"""
    return C.make_inputs(**dict(C.G1_INPUTS, n_img=N_IMG, seed=int(seed)))
