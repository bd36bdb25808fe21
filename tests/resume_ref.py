"""Constants of golden G18 (tests/golden/make_golden_resume.py): the reference's resume flow on the tiny models.

A case runs steps 0 and 1, takes ``copy.deepcopy(opt.state_dict())``, builds a NEW ``get_optim`` optimiser over the same model, loads
that dict into it (``maybe_load_checkpoint``, utils/training.py:181-185) and runs steps 2 and 3.  The new wrapper's ``_step`` and the
loop's ``global_step`` start at 0 again (``prepare()``, utils/training.py:136), so the rate schedule and the sparsity-loss ramp restart
while the inner ``torch.optim`` state — the moments and Adam's ``step`` — continues.

The generator, the host tests (tests/test_resume_host.py) and the device tests (tests/test_gpu_resume.py) all read this table."""
import optim_ref as R

G18_STEPS, G18_SPLIT, G18_CLIP = 4, 2, R.G17_CLIP
# name -> the reference's config names that differ from G17_DEFAULTS (tests/optim_ref.py).  The rates are G17's; one constant differs, see
# below: every stored tensor of the resumed run has to lie at least MIN_DIFF away from the same run with a fresh second optimiser
# and, where the schedule depends on the step, from the uninterrupted run (asserted by the generator).
G18_DENSE = {
    "noam_adam": dict(lr_scheduler="noam", optim="adam"),
    "step_sgdm": dict(lr_scheduler="step", optim="sgdm", learning_rate=0.5),
    # G17's rmsprop case runs with optim_epsilon 1e-2; there a small gradient (the WG weights') moves its weight by lr * g / eps whatever
    # square_avg holds, 9e-4 between a loaded and a fresh optimiser.  At the reference's default epsilon (1e-8) the state decides.
    "cosine_rmsprop": dict(lr_scheduler="cosine", optim="rmsprop", learning_rate=0.02, max_train_step=4),
}
G18_MASKED = {
    "masked_step_adam": dict(lr_scheduler="step", optim="adam", learning_rate=0.02, optim_beta=0.98, optim_epsilon=1e-9),
}
G18_MASK = dict(lr_mask=100.0, target=0.9, weight=30.0)
G18_PARAMS, G18_MASK_PARAM = R.G17_PARAMS, R.G17_MASK_PARAM
MIN_DIFF = 1e-2            # 20 x the 5e-4 comparison bar
STEP_SCHEDULES = ("noam", "cosine")          # the rate depends on the wrapper's step count: resumed != uninterrupted


def g18_config(case):
    over = G18_DENSE.get(case) or G18_MASKED[case]
    return dict(R.G17_DEFAULTS, **over)
