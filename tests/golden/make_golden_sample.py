#!/usr/bin/env python3
"""Golden fixture G14: the kept sets of the reference's truncated sampling, CaptionModel.sample_next_word with "top<k>" / "top<p>"
(sparse_caption/models/caption_model.py:246-266), on seeded log-prob rows.
    python tests/golden/make_golden_sample.py      # writes tests/golden/g14_sample_truncate.npz
The method draws with torch.distributions.Categorical(logits=...): those logits are -inf exactly outside the kept set, so the class
is replaced, inside this script, by a recorder, and the fixture stores the inputs and the finite-mask of the recorded logits (the
draw itself follows torch's RNG stream and is not part of the fixture)."""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

CASES = (("top3", 1.0), ("top5", 0.9), ("top0.8", 1.0), ("top0.5", 1.3))      # (sample_method, temperature)
ROWS, VOCAB, SEED = 16, 101, 1414


def inputs():
    import torch
    g = torch.Generator().manual_seed(SEED)
    return torch.log_softmax(2.0 * torch.randn(ROWS, VOCAB, generator=g), -1)


def main():
    import torch
    import_reference()
    from sparse_caption.models.caption_model import CaptionModel
    seen = []

    class Recorder:
        def __init__(self, logits):
            seen.append(logits.clone())

        def sample(self):
            return seen[-1].argmax(-1)

    real = torch.distributions.Categorical
    torch.distributions.Categorical = Recorder
    try:
        g = {"logprobs": inputs().numpy()}
        assert len(np.unique(g["logprobs"])) == ROWS * VOCAB      # no exact ties: the order does not depend on a tie rule
        for method, temperature in CASES:
            CaptionModel.sample_next_word(inputs(), method, temperature)
            keep = torch.isfinite(seen[-1]).numpy()
            g[f"{method}/temperature"] = np.float32(temperature)
            g[f"{method}/keep_bits"] = np.packbits(keep.reshape(-1))
            print(method, temperature, "kept per row:", keep.sum(1).tolist())
    finally:
        torch.distributions.Categorical = real
    np.savez_compressed(os.path.join(HERE, "g14_sample_truncate.npz"), **g)


if __name__ == "__main__":
    main()
