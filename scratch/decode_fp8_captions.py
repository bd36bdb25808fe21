"""What FP8 weight quantisation of the decoder costs the captions (recorded, not asserted), on the inputs of
tests/test_gpu_decode_fp8.py: FULL_CFG with `margin_state` weights (RANDOM weights with real decision margins — no trained checkpoint),
70 images x 12-36 regions and 37 images x 33-100 regions, greedy and beam 5 — and the same with the EOS bias taken out, which makes the
captions of these random-weight models long and different per image.
  * GPU: `executor="stack_fp8"` against `executor="stack"` on the unquantised weights W: share of identical best captions, mean and
    max |difference of log-probs| over agreeing tokens of the best captions;
  * CPU, fp32 oracle (oracle/ort_oracle.py) on W against the oracle on W' = fp8_dequantized_decoder_state() — the part that is due to
    quantisation alone, no bf16 arithmetic in it — on the first `--oracle-images` images of the 36-region batch (the oracle is slow).
Prints lines for profiles/decode_fp8.txt."""
import argparse, os, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (HERE, os.path.join(HERE, "tests"), os.path.join(HERE, "tests", "golden")):
    sys.path.insert(0, p)


def figures(s_a, l_a, s_b, l_b):
    """best captions (N, L) of two decodes -> (share identical, mean |dlp|, max |dlp| over agreeing non-pad tokens)"""
    same_cap = (s_a == s_b).all(-1).float().mean().item()
    tok = (s_a == s_b) & (s_a != 0)
    d = (l_a - l_b)[tok].abs()
    return same_cap, d.mean().item(), d.max().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--oracle-images", type=int, default=70)
    a = ap.parse_args()
    import torch
    import common as C
    import helpers as H
    import sparse_image_captioning_amd as pkg
    from sparse_image_captioning_amd.utils.config import Config
    from oracle import ort_oracle as O
    pkg._lib.require_gpu()
    cfg = O.OCfg(**{k: v for k, v in C.FULL_CFG.items() if not k.startswith("prune")})
    n = a.oracle_images
    print("captions under FP8 decoder weights; RANDOM weights, no trained checkpoint.  margin_state = generator x 3 + EOS bias (best captions end "
          "at once); long = generator x 3, no EOS bias (16-token captions, different per image)")
    for wname, eos_bias in (("margin_state", C.G1_EOS_BIAS), ("long", 0.0)):
        state = H.torch_state(H.dense_param_shapes(C.FULL_CFG), C.G2_SEED, C.G1_GEN_SCALE, eos_bias)
        m = pkg.get_model("relation_transformer")(Config(**C.FULL_CFG), precision=1)
        m.load_state_dict(state, strict=False)
        m = m.cuda().eval()
        cpu_b = None
        for n_reg, n_img in ((36, 70), (100, 37)):
            cb = H.torch_batch(C.make_inputs(seed=41, n_img=n_img, n_reg=n_reg, feat=2048, vocab=10001, spi=1, ragged=True))
            cpu_b = cpu_b or cb
            b = {k: v.cuda() for k, v in cb.items()}
            for beam in (1, 5):
                out = {}
                for ex in ("stack", "stack_fp8"):
                    with torch.no_grad():
                        seq, lp = m(att_feats=b["att_feats"], boxes=b["boxes"], att_masks=b["att_masks"], opt={"beam_size": beam, "executor": ex}, mode="sample")
                    out[ex] = (seq[:, 0].cpu(), lp[:, 0].cpu())
                f = figures(*out["stack"], *out["stack_fp8"])
                print(f"{wname:12s} GPU  stack_fp8 vs stack on W   {n_img:3d} images x {n_reg:3d} regions beam {beam}: identical best captions {f[0]:.3f}   "
                      f"|dlogp| over agreeing tokens mean {f[1]:.4f} max {f[2]:.4f}   mean length {(out['stack'][0] != 0).sum(-1).float().mean().item():.1f}")
        deq = {k: v.cpu() for k, v in m.fp8_dequantized_decoder_state().items()}
        sub = {k: v[:n] for k, v in cpu_b.items() if k in ("att_feats", "boxes", "att_masks")}
        for beam in (1, 5):
            out = []
            for P in (state, dict(state, **deq)):
                with torch.no_grad():
                    if beam == 1:
                        seq, lp = O.sample_greedy_or_multinomial(P, cfg, sub["att_feats"], sub["boxes"], sub["att_masks"])[:2]
                    else:
                        seq, lp, _ = O.beam_search(P, cfg, sub["att_feats"], sub["boxes"], sub["att_masks"], beam)
                out.append((seq.view(n, -1, seq.size(-1))[:, 0], lp.view(n, -1, lp.size(-1))[:, 0]))
            f = figures(*out[0], *out[1])
            print(f"{wname:12s} CPU  fp32 oracle on W' vs on W  {n:3d} images x  36 regions beam {beam}: identical best captions {f[0]:.3f}   "
                  f"|dlogp| over agreeing tokens mean {f[1]:.4f} max {f[2]:.4f}")
        del m

if __name__ == "__main__":
    main()
