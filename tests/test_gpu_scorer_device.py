"""Device-side SCST reward (csrc/ortk_scorer_dev.hip through CaptionScorer.device_refs / score_device): against golden G6 (the
reference's own scorer), against the host scorer at benchmark size, bit-for-bit determinism, and end to end through
NativeTrainer.scst_step.  Tolerances: 1e-9 relative / 1e-12 absolute on the fp64 scores (fp64 with another libm: what the host
tests use against the same golden; the sums have at most a few hundred positive terms); the fp32 reward at 1e-5 / 1e-6 (the
figures tests/test_scorer_host.py uses for the trainer's reward function)."""
import numpy as np
import pytest
import torch

import common as C
import helpers as H
import scorer_inputs as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import sparse_image_captioning_amd as pkg
    pkg._lib.require_gpu()
    return pkg


def _device_scores(sc, refs, sample, greedy, eos=S.EOS, pad=S.PAD):
    dev = torch.device("cuda:0")
    s = torch.from_numpy(sample).to(dev)
    g = None if greedy is None else torch.from_numpy(greedy).to(dev)
    dr = sc.device_refs(refs, sample.shape[1] + (g is not None), dev, vocab_size=101)
    reward, scs, scb = sc.score_device(dr, s, g, eos_idx=eos, pad_idx=pad)
    assert reward.is_cuda and reward.dtype == torch.float32 and scs.dtype == scb.dtype == torch.float64
    return reward.cpu().numpy(), scs.cpu().numpy(), scb.cpu().numpy()


def test_device_scorer_matches_golden_g6(P):
    from sparse_image_captioning_amd.scst import CaptionScorer
    g6 = S.g6()
    id_table, ref_ids, sample, greedy = S.g6_id_space(g6)
    ns = sample.shape[1]
    assert len(g6["cases"]) == 6
    for case in g6["cases"]:
        sc = CaptionScorer(id_table, cider_weight=case["cider_weight"], bleu_weight=case["bleu_weight"])
        reward, s, b = _device_scores(sc, ref_ids, sample, greedy if case["baseline"] else None)
        print("g6 case", case["cider_weight"], case["bleu_weight"], case["baseline"], "max rel",
              float(np.max(np.abs(s - case["sc_sample"]) / np.maximum(np.abs(case["sc_sample"]), 1e-300))))
        np.testing.assert_allclose(s, case["sc_sample"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(b, case["sc_baseline"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(reward, (s - b).astype(np.float32), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(reward, (np.array(case["sc_sample"]) - np.array(case["sc_baseline"])).astype(np.float32),
                                   rtol=1e-5, atol=1e-6)
    sc = CaptionScorer("corpus", cider_weight=1.0)
    reward, s, b = _device_scores(sc, ref_ids, sample, greedy)
    want = np.array(g6["corpus_cider_items"])
    nb = len(g6["baseline"])
    np.testing.assert_allclose(s, want[nb:], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(b, np.repeat(want[:nb], ns), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(reward, (s - b).astype(np.float32), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("L,n_images,seed", [(18, 256, 1), (64, 32, 2)])
def test_device_scorer_matches_host_scorer_at_bench_size(P, L, n_images, seed):
    """256 images x (5 samples + greedy) at L = 18 (the benchmark's shape), and L = 64 with 32 images; cached table and corpus
    mode, both baselines, both weightings.  EVERY row is compared."""
    from sparse_image_captioning_amd.scst import CaptionScorer
    ns = 5
    refs, sample, greedy, caps = S.random_batch(seed, n_images, ns, L)
    table = S.random_table(refs, seed)
    S.assert_input_conditions(table, refs, sample, greedy, caps, L)
    for src in (table, "corpus"):
        for wc, wb in S.WEIGHTS:
            for baseline in ("greedy", "leave_one_out"):
                want_s, want_b = S.host_scores(src, refs, sample, greedy, wc, wb, baseline)
                sc = CaptionScorer(src, cider_weight=wc, bleu_weight=wb)
                reward, s, b = _device_scores(sc, refs, sample, greedy if baseline == "greedy" else None)
                assert s.shape == want_s.shape == (n_images * ns,) and reward.shape == s.shape
                print("L", L, "corpus" if src == "corpus" else "cached", wc, wb, baseline, "max abs diff sample / baseline",
                      float(np.abs(s - want_s).max()), float(np.abs(b - want_b).max()))
                np.testing.assert_allclose(s, want_s, rtol=1e-9, atol=1e-12)
                np.testing.assert_allclose(b, want_b, rtol=1e-9, atol=1e-12)
                np.testing.assert_allclose(reward, (want_s - want_b).astype(np.float32), rtol=1e-5, atol=1e-6)


def test_device_scorer_is_deterministic(P):
    from sparse_image_captioning_amd.scst import CaptionScorer
    refs, sample, greedy, _ = S.random_batch(1, 256, 5, 18)
    dev = torch.device("cuda:0")
    s, g = torch.from_numpy(sample).to(dev), torch.from_numpy(greedy).to(dev)
    for src in (S.random_table(refs, 1), "corpus"):
        sc = CaptionScorer(src, cider_weight=0.5, bleu_weight=[0.1, 0.2, 0.3, 0.4])
        for gg in (g, None):
            dr = sc.device_refs(refs, 5 + (gg is not None), dev, vocab_size=101)
            a = [t.clone() for t in sc.score_device(dr, s, gg)]
            b = sc.score_device(sc.device_refs(refs, 5 + (gg is not None), dev), s, gg)
            assert float(a[1].abs().sum()) > 0
            for x, y in zip(a, b):
                assert torch.equal(x, y)          # bit-identical: no atomics, fixed-order reductions


def test_device_scorer_refuses_what_it_cannot_score(P):
    from sparse_image_captioning_amd.scst import CaptionScorer
    from sparse_image_captioning_amd.training import NativeTrainer
    g6 = S.g6()
    id_table, ref_ids, sample, greedy = S.g6_id_space(g6)
    word_table = {"document_frequency": {tuple(k): v for k, v in g6["df"]}, "ref_len": g6["ref_len"]}
    with pytest.raises(ValueError):               # raw token ids against a word-keyed table: as score_sequences without `decode`
        CaptionScorer(word_table, cider_weight=1.0).device_refs(ref_ids, 4, "cuda:0")
    sc = CaptionScorer(id_table, cider_weight=1.0)
    with pytest.raises(ValueError):               # the kernel cannot report an id it cannot pack
        sc.device_refs(ref_ids, 4, "cuda:0", vocab_size=65535)
    with pytest.raises(ValueError):
        NativeTrainer.scorer_reward_fn(sc, ref_ids, device=True, vocab_size=70000)
    dr = sc.device_refs(ref_ids, 4, "cuda:0", vocab_size=65534)
    with pytest.raises(ValueError):               # cooked for samples + greedy, called without the greedy rows
        sc.score_device(dr, torch.from_numpy(sample).cuda(), None)
    with pytest.raises(ValueError):               # host tensors
        sc.score_device(dr, torch.from_numpy(sample), torch.from_numpy(greedy))


@pytest.mark.parametrize("baseline", ["greedy", "leave_one_out"])
def test_scst_step_with_device_reward_equals_host_reward(P, baseline):
    """Two trainers from the same weights and seeds, one SCST step each: host CaptionScorer reward against device=True.  The
    only difference between the two steps is the fp32 rounding of the reward."""
    from sparse_image_captioning_amd.scst import CaptionScorer
    from sparse_image_captioning_amd.training import NativeTrainer
    from sparse_image_captioning_amd.utils.config import Config
    ns = 3
    cb = H.g1_batch()
    N = cb["att_feats"].size(0)
    rs = np.random.RandomState(3)
    refs = [[[int(t) for t in rs.randint(4, 60, size=rs.randint(5, 12))] for _ in range(3)] for _ in range(N)]
    out = {}
    for kind in ("host", "device"):
        torch.manual_seed(4321)
        m = P.get_model("relation_transformer")(Config(**C.TINY_CFG))
        m.load_state_dict(H.g1_state(), strict=False)      # (generator scaled, EOS biased: tests/golden/common.py — captions end)
        m = m.cuda().eval()
        b = {k: v.cuda() for k, v in cb.items()}
        scorer = CaptionScorer("corpus", cider_weight=1.0, bleu_weight=[0.0, 0.0, 0.0, 0.5])
        fn = NativeTrainer.scorer_reward_fn(scorer, refs, eos_idx=C.EOS, pad_idx=C.PAD, device=kind == "device",
                                            vocab_size=C.TINY_CFG["vocab_size"] if kind == "device" else None)
        tr = NativeTrainer(m, noamopt_factor=1.0, noamopt_warmup=10, keep_grads=True)
        tr.valid_positions = False
        m._seed_counter = 20
        loss, reward, seq, greedy = tr.scst_step(b, fn, num_samples=ns, baseline=baseline, train=False)
        assert reward.is_cuda
        out[kind] = (float(loss), reward.cpu().numpy(), seq.cpu(), None if greedy is None else greedy.cpu())
        assert fn(seq, greedy).is_cuda == (kind == "device")      # the device reward never leaves the GPU
    (lh, rh, sh, gh), (ld, rd, sd, gd) = out["host"], out["device"]
    assert torch.equal(sh, sd), "sampled tokens"
    assert (gh is None and gd is None) if baseline != "greedy" else torch.equal(gh, gd), "greedy tokens"
    lens = (sh != C.PAD).sum(-1)
    assert int(lens.min()) < sh.size(-1) and float(np.abs(rh).max()) > 1e-3      # captions end, rewards are not all zero
    print("baseline", baseline, "reward max abs diff", float(np.abs(rh - rd).max()), "loss host / device", lh, ld)
    np.testing.assert_allclose(rd, rh, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ld, lh, rtol=1e-5)
