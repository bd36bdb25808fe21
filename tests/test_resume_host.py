"""Host-side checks of save / resume (no GPU): the reference-format optimiser state against live ``torch.optim`` instances, every
refusal of the two loaders, the reference's parameter order against golden G18 (tests/golden/make_golden_resume.py), the rank logic
and the atomic write of the checkpoint files."""
import copy
import os
import warnings

import pytest
import torch

import common as C
import optim_ref as R
import resume_ref as RR

KINDS_WITH_STATE = [k for k in R.KINDS if R.N_STATES[k] > 0]
NAMES = ["w", "b", "t"]
SHAPES = {"w": (3, 5), "b": (7,), "t": (2, 2, 2)}


@pytest.fixture(scope="module")
def S():
    import sparse_image_captioning_amd.optim_state as S
    return S


def _spec(kind, scheduler="step", **kw):
    from sparse_image_captioning_amd.training import OptimSpec
    return OptimSpec(8, noamopt_warmup=10, max_train_step=10, optim=kind, lr_scheduler=scheduler, learning_rate=0.05, optim_alpha=0.9,
                     optim_beta=0.99, optim_epsilon=1e-6, **kw)


def _reference_optimizer(kind, params, spec, wd=0.0):
    """The constructor calls of the reference's build_optimizer (utils/optim.py:149-174), written out here independently of
    optim_state.build_torch_optimizer."""
    lr, a, b, eps = spec.learning_rate, spec.alpha, spec.beta, spec.eps
    if kind == "adam":
        return torch.optim.Adam(params, lr, (a, b), eps, weight_decay=wd)
    if kind == "sgd":
        return torch.optim.SGD(params, lr, weight_decay=wd)
    if kind == "sgdm":
        return torch.optim.SGD(params, lr, a, weight_decay=wd)
    if kind == "sgdmom":
        return torch.optim.SGD(params, lr, a, weight_decay=wd, nesterov=True)
    if kind == "rmsprop":
        return torch.optim.RMSprop(params, lr, a, eps, weight_decay=wd)
    return torch.optim.Adagrad(params, lr, weight_decay=wd)


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(SHAPES[n], generator=g)) for n in NAMES]


def _grads(step):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(SHAPES[n], generator=g) for n in NAMES]


def _take(opt, params, step):
    for p, g in zip(params, _grads(step)):
        p.grad = g.clone()
    opt.step()


@pytest.mark.parametrize("kind", KINDS_WITH_STATE)
def test_state_through_unpack_and_pack_continues_a_live_optimiser_bitwise(S, kind):
    spec = _spec(kind)
    p1 = _params()
    o1 = _reference_optimizer(kind, p1, spec)
    _take(o1, p1, 0)
    _take(o1, p1, 1)
    state, mask_state, step = S.unpack_optimizer_state(spec, copy.deepcopy(o1.state_dict()), [NAMES], SHAPES)
    assert mask_state is None and step == (None if kind in S.STEPLESS else 2)
    assert sorted(state) == sorted(S.STATE_ARRAYS[kind]) and all(sorted(v) == sorted(NAMES) for v in state.values())
    optim_step, _ = S.resolve_steps(spec, step, 0)
    packed = S.pack_optimizer_state(spec, [NAMES], SHAPES, state, None, optim_step, lr=spec.learning_rate)
    p2 = [torch.nn.Parameter(p.detach().clone()) for p in p1]
    o2 = _reference_optimizer(kind, p2, spec)
    o2.load_state_dict(packed)
    before = [p.detach().clone() for p in p1]
    _take(o1, p1, 2)
    _take(o2, p2, 2)
    for a, b, c in zip(p1, p2, before):
        assert torch.equal(a, b) and not torch.equal(a, c)
    # ... and the loaded state mattered: a second optimiser that was not loaded ends elsewhere
    p3 = [torch.nn.Parameter(c.clone()) for c in before]
    o3 = _reference_optimizer(kind, p3, spec)
    _take(o3, p3, 2)
    assert not all(torch.equal(a, b) for a, b in zip(p1, p3))


def _kinds_of(entry):
    return {k: (type(v), getattr(v, "dtype", None), tuple(getattr(v, "shape", ())), str(getattr(v, "device", ""))) for k, v in entry.items()}


@pytest.mark.parametrize("kind", R.KINDS)
def test_pack_from_nothing_has_the_keys_and_types_torch_writes(S, kind):
    spec = _spec(kind)
    packed = S.pack_optimizer_state(spec, [NAMES], SHAPES)
    params = _params()
    live = _reference_optimizer(kind, params, spec)
    _take(live, params, 0)
    want = live.state_dict()
    assert sorted(packed) == sorted(want) and sorted(packed["state"]) == sorted(want["state"])
    for i in want["state"]:
        assert _kinds_of(packed["state"][i]) == _kinds_of(want["state"][i]) and list(packed["state"][i]) == list(want["state"][i])
    assert len(packed["param_groups"]) == 1
    assert {k: type(v) for k, v in packed["param_groups"][0].items()} == {k: type(v) for k, v in want["param_groups"][0].items()}
    assert packed["param_groups"][0] == want["param_groups"][0]
    # the two-group layout of a supermask model: what torch makes of the reference's group dicts
    names = [NAMES, ["w_pruning_mask"]]
    shapes = dict(SHAPES, w_pruning_mask=SHAPES["w"])
    two = S.pack_optimizer_state(spec, names, shapes, mask_lr=100.0, mask_eps=1e-2, optim_step=3)
    params, mask = _params(), torch.nn.Parameter(torch.zeros(SHAPES["w"]))
    live = _reference_optimizer(kind, [{"params": params}, {"params": [mask], "lr": 100.0, "weight_decay": 0, "eps": 1e-2,
                                                           "pruning_mask": True}], spec)
    assert two["param_groups"] == live.state_dict()["param_groups"]
    assert sorted(two["state"]) == ([] if kind == "sgd" else [0, 1, 2, 3])
    if kind not in S.STEPLESS:
        assert all(int(e["step"]) == 3 for e in two["state"].values())
    S.unpack_optimizer_state(spec, two, names, shapes, mask_lr=100.0, mask_eps=1e-2)


def test_noam_builds_the_references_adam(S):
    spec = _spec("sgd", scheduler="noam")
    g = S.pack_optimizer_state(spec, [NAMES], SHAPES)["param_groups"][0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (0, (0.9, 0.98), 1e-9, 0)           # utils/optim.py:122


# ---------------------------------------------------------------------------------------------- refusals
def _good(S, kind="adam", masked=False):
    spec = _spec(kind)
    names = [NAMES, ["w_pruning_mask"]] if masked else [NAMES]
    shapes = dict(SHAPES, w_pruning_mask=SHAPES["w"])
    return spec, names, shapes, S.pack_optimizer_state(spec, names, shapes, optim_step=2)


def test_reference_format_refusals(S):
    spec, names, shapes, d = _good(S)
    S.unpack_optimizer_state(spec, d, names, shapes)

    def refused(match, change, spec=spec, names=names, shapes=shapes, kind="adam", masked=False):
        _, _, _, fresh = _good(S, kind, masked)
        change(fresh)
        with pytest.raises(ValueError, match=match):
            S.unpack_optimizer_state(spec, fresh, names, shapes)

    for key, value in (("amsgrad", True), ("maximize", True)):
        refused(key, lambda d, k=key, v=value: d["param_groups"][0].__setitem__(k, v))
    for key, value in (("centered", True),):
        refused(key, lambda d, k=key, v=value: d["param_groups"][0].__setitem__(k, v), spec=_spec("rmsprop"), kind="rmsprop")
    for key, value in (("lr_decay", 0.1), ("initial_accumulator_value", 0.5)):
        refused(key, lambda d, k=key, v=value: d["param_groups"][0].__setitem__(k, v), spec=_spec("adagrad"), kind="adagrad")
    # group layouts that do not fit the model
    refused("group", lambda d: d["param_groups"].append(dict(d["param_groups"][0], params=[3])))
    refused("group", lambda d: None, names=[NAMES, ["w_pruning_mask"]])                    # a dense file into a supermask trainer
    refused("group", lambda d: None, masked=True)                                          # a supermask file into a dense trainer
    refused("param group 0", lambda d: d["param_groups"][0].__setitem__("params", [0, 1]))
    refused("pruning_mask", lambda d: d["param_groups"][1].pop("pruning_mask"), names=[NAMES, ["w_pruning_mask"]], masked=True)
    # constants of the file that are not this trainer's, a missing entry, a missing array, a shape
    refused("betas", lambda d: d["param_groups"][0].__setitem__("betas", (0.9, 0.5)))
    refused("eps", lambda d: d["param_groups"][0].__setitem__("eps", 1e-3))
    refused("weight_decay", lambda d: d["param_groups"][0].__setitem__("weight_decay", 0.1))
    refused("momentum", lambda d: None, spec=_spec("sgd"), kind="sgdm")
    refused("'b'", lambda d: d["state"].pop(1))
    refused("exp_avg_sq", lambda d: d["state"][2].pop("exp_avg_sq"))
    refused(r"\(7,\)", lambda d: d["state"][1].__setitem__("exp_avg", torch.zeros(8)))
    refused("step counts", lambda d: d["state"][0].__setitem__("step", torch.tensor(5.0)))
    refused("unknown parameter", lambda d: d["state"].__setitem__(9, dict(d["state"][0])))
    with pytest.raises(ValueError, match="param_groups"):
        S.unpack_optimizer_state(spec, {"format": 1}, names, shapes)


def test_rate_step_rules(S):
    assert S.resolve_steps(_spec("adam"), 7, None) == (7, 7)           # the uninterrupted schedule
    assert S.resolve_steps(_spec("adam"), 7, 0) == (7, 0)              # the reference's resume: the wrapper counts from 0
    assert S.resolve_steps(_spec("sgdm"), None, 0) == (1, 0)           # a loaded momentum_buffer: not the first step
    assert S.resolve_steps(_spec("sgd"), None, 4) == (0, 4)
    for kind in S.STEPLESS:
        with pytest.raises(ValueError, match="rate_step"):
            S.resolve_steps(_spec(kind), None, None)
    with pytest.raises(ValueError, match="negative"):
        S.resolve_steps(_spec("adam"), 7, -1)


def _native(S, spec, names, mask_names=None, **over):
    arrays = S.STATE_ARRAYS[spec.kind]
    shapes = dict(SHAPES, w_pruning_mask=SHAPES["w"])
    sd = dict(format=S.FORMAT, spec=S.spec_fields(spec), rate_step=2, optim_step=2, epoch=0, seed=dict(base=1, counter=2),
              options=dict(grad_clip=0.1), state={a: {n: torch.zeros(shapes[n]) for n in names} for a in arrays})
    if mask_names is not None:
        sd["mask_state"] = {a: {n: torch.zeros(shapes[n]) for n in mask_names} for a in arrays}
    sd.update(over)
    return sd, shapes


def test_native_format_refusals_and_the_one_warning(S):
    spec = _spec("adam")
    sd, shapes = _native(S, spec, NAMES)
    opts = dict(grad_clip=0.1)
    assert S.check_native_state(sd, spec, NAMES, shapes, None, opts) == []

    def refused(match, sd, spec=spec, names=NAMES, mask_names=None):
        with pytest.raises(ValueError, match=match):
            S.check_native_state(sd, spec, names, shapes, mask_names, opts)

    refused("format.*2.*1", dict(sd, format=2))
    refused("format", [1, 2])
    refused("optim_step: missing", {k: v for k, v in sd.items() if k != "optim_step"})
    refused("seed: missing", {k: v for k, v in sd.items() if k != "seed"})
    refused("kind.*adam.*rmsprop", sd, spec=_spec("rmsprop"))
    refused("scheduler.*step.*cosine", sd, spec=_spec("adam", scheduler="cosine"))
    refused("weight_decay.*0.0.*0.01", sd, spec=_spec("adam", weight_decay=0.01))
    other = _spec("adam")
    other.eps = 1e-3
    refused("eps.*1e-06.*0.001", sd, spec=other)
    refused("missing.*'u'", sd, names=NAMES + ["u"])
    refused("unexpected.*'t'", sd, names=NAMES[:2])
    bad = _native(S, spec, NAMES)[0]
    bad["state"]["exp_avg"]["b"] = torch.zeros(8)
    refused(r"exp_avg\['b'\].*\(8,\).*\(7,\)", bad)
    refused("masked / dense", sd, mask_names=["w_pruning_mask"])
    refused("masked / dense", _native(S, spec, NAMES, ["w_pruning_mask"])[0])
    refused("mask_state.exp_avg.*missing", _native(S, spec, NAMES, [])[0], mask_names=["w_pruning_mask"])
    # informational options: listed, not refused, and ONE warning for all of them
    diff = S.check_native_state(dict(sd, options=dict(grad_clip=0.5)), _spec("adam", learning_rate_decay_every=5), NAMES, shapes, None, opts)
    assert len(diff) == 2 and "grad_clip" in diff[1] and "decay_every" in diff[0]
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        S.warn_differences(diff)
        S.warn_differences([])
    assert len(seen) == 1 and "grad_clip" in str(seen[0].message) and "decay_every" in str(seen[0].message)


def test_the_trainers_loaders_refuse_before_any_device_work(S):
    """A trainer shell around a CPU model with NO arenas at all: a loader that touched one before its checks were through would die
    of an AttributeError, not of the ValueError."""
    from sparse_image_captioning_amd import get_model
    from sparse_image_captioning_amd.training import NativeTrainer, OptimSpec
    from sparse_image_captioning_amd.utils.config import Config
    model = get_model("relation_transformer")(Config(**C.TINY_CFG))
    tr = object.__new__(NativeTrainer)
    tr.model, tr.masked, tr.spec = model, False, OptimSpec(model.d_model, optim="sgdm", lr_scheduler="step")
    tr.clip, tr.label_smoothing, tr.max_train_step, tr.step_count, tr.epoch = 0.1, 0.0, 1, 0, 0
    names = tr.optimizer_group_names()
    shapes = {e["name"]: e["shape"] for e in model.named_weight_entries()}
    good = S.pack_optimizer_state(tr.spec, names, shapes)
    with pytest.raises(ValueError, match="rate_step"):
        tr.load_optimizer_state_dict(good)                                    # sgdm stores no step
    good["param_groups"][0]["maximize"] = True
    with pytest.raises(ValueError, match="maximize"):
        tr.load_optimizer_state_dict(good, rate_step=0)
    with pytest.raises(ValueError, match="format"):
        tr.load_state_dict({"format": 0})
    sd, _ = _native(S, tr.spec, [])
    with pytest.raises(ValueError, match="missing"):
        tr.load_state_dict(sd)
    with pytest.raises(AttributeError):                                       # (the shell really has no arenas: a good state gets that far)
        good["param_groups"][0]["maximize"] = False
        tr.load_optimizer_state_dict(good, rate_step=0)


# ---------------------------------------------------------------------------------------------- the reference's parameter order
def _entries(name, cfg):
    from sparse_image_captioning_amd import get_model
    from sparse_image_captioning_amd.utils.config import Config
    return get_model(name)(Config(**cfg)).named_weight_entries()


def test_group_names_dense_vs_reference_golden(S, golden):
    g18 = golden("g18_tiny_resume")
    got = S.group_names(_entries("relation_transformer", C.TINY_CFG))
    for case in RR.G18_DENSE:
        assert int(g18[f"{case}/n_groups"]) == 1
        assert got == [[str(n) for n in g18[f"{case}/group0_names"]]]
    assert got[0] != [e["name"] for e in _entries("relation_transformer", C.TINY_CFG)]        # (the arena's own order is another)


def test_group_names_masked_vs_reference_golden(S, golden):
    g18 = golden("g18_tiny_resume")
    cfg = dict(C.TINY_CFG, prune_type="supermask", prune_mask_freeze_scope="model.generator.", prune_supermask_init=5.0)
    got = S.group_names(_entries("relation_transformer_prune", cfg), True, ["model.generator."])
    assert int(g18["masked_step_adam/n_groups"]) == 2
    assert got == [[str(n) for n in g18[f"masked_step_adam/group{i}_names"]] for i in range(2)]
    assert not any(n.startswith("model.generator.") for n in got[1]) and all(n.endswith("_pruning_mask") for n in got[1])


def test_group_names_shared_layers_and_plain_transformer_vs_reference_goldens(S, golden):
    """The orders the reference recorded in goldens G8 (ACORT layer sharing: a shared parameter once) and G10 (plain transformer)."""
    g8 = golden("g8_tiny_share_layer")
    cfg = dict(C.TINY_CFG, num_layers=3, share_layer_encoder=(0, 1, 0), share_layer_decoder=(0, 0, 1))
    assert S.group_names(_entries("relation_transformer", cfg)) == [[str(n) for n in g8["param_names"]]]
    g10 = golden("g10_tiny_plain_transformer")
    got = S.group_names(_entries("transformer", C.TINY_CFG))
    assert got == [[str(n) for n in g10["param_names"]]]
    with pytest.raises(ValueError, match="no place"):
        S.group_names([dict(name="model.encoder.surprise.weight", kind=0)])


# ---------------------------------------------------------------------------------------------- files
def _files(tmp_path, tag="last"):
    from sparse_image_captioning_amd.optim_state import checkpoint_paths
    return checkpoint_paths(str(tmp_path), tag)


def test_checkpoint_file_names_are_the_references(tmp_path):
    assert [os.path.basename(p) for p in _files(tmp_path)] == ["model_last.pth", "optimizer_last.pth", "trainer_last.pth"]
    assert [os.path.basename(p) for p in _files(tmp_path, "best")] == ["model_best.pth", "optimizer_best.pth", "trainer_best.pth"]


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 4), (1, 4), (3, 4)])
def test_only_rank_0_writes(S, tmp_path, monkeypatch, rank, world):
    from sparse_image_captioning_amd import parallel
    monkeypatch.setattr(parallel, "rank", lambda: rank)
    monkeypatch.setattr(parallel, "world", lambda: world)
    waited = []
    monkeypatch.setattr(parallel, "barrier", lambda: waited.append(1))
    made = []
    paths = _files(tmp_path)

    def make():
        made.append(1)
        return {p: {"x": torch.full((3,), float(i))} for i, p in enumerate(paths)}
    S.write_files(make)
    assert waited == [1]                                     # every rank reaches the barrier, after the write
    if rank == 0:
        assert made == [1] and sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for p in paths)
        assert [float(S.read_file(p)["x"][0]) for p in paths] == [0.0, 1.0, 2.0]
    else:
        assert made == [] and os.listdir(tmp_path) == []     # the state is not even gathered


def test_a_killed_write_leaves_the_previous_checkpoint_whole(S, tmp_path, monkeypatch):
    paths = _files(tmp_path)
    S.write_files(lambda: {p: {"x": torch.full((3,), float(i))} for i, p in enumerate(paths)})
    before = {p: open(p, "rb").read() for p in paths}
    real, calls = torch.save, []

    def dying(obj, f, *a, **k):
        calls.append(f)
        if len(calls) == 2:                                  # the second file: half written, then the process "dies"
            with open(f, "wb") as fh:
                fh.write(b"half a file")
            raise KeyboardInterrupt
        return real(obj, f, *a, **k)
    monkeypatch.setattr(torch, "save", dying)
    with pytest.raises(KeyboardInterrupt):
        S.write_files(lambda: {p: {"x": torch.full((3,), 9.0)} for p in paths})
    monkeypatch.setattr(torch, "save", real)
    assert len(calls) == 2 and not any(c in paths for c in calls)          # nothing is ever written under a final name
    assert {p: open(p, "rb").read() for p in paths} == before               # not even the first, complete, file was renamed
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for p in paths)       # and no partial file is left
    S.write_files(lambda: {p: {"x": torch.full((3,), 9.0)} for p in paths})
    assert all(float(S.read_file(p)["x"][0]) == 9.0 for p in paths)


def test_native_state_survives_weights_only_load(S, tmp_path):
    spec = _spec("adam")
    sd, _ = _native(S, spec, NAMES, ["w_pruning_mask"])
    path = os.path.join(str(tmp_path), "trainer_last.pth")
    torch.save(sd, path)
    back = S.read_file(path)                                  # torch.load(..., weights_only=True)
    assert back["spec"] == sd["spec"] and back["seed"] == sd["seed"] and sorted(back) == sorted(sd)
    assert all(torch.equal(back["state"][a][n], sd["state"][a][n]) for a in sd["state"] for n in NAMES)
