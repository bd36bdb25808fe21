"""Optimiser state off the device: the two formats a ``NativeTrainer`` saves and loads, and the checkpoint files.

  native     ``NativeTrainer.state_dict()``: a plain dict of ints, floats, strings and CPU fp32 tensors keyed by PARAMETER NAME (the
             ``ortk_arena_entry`` names = the reference's state_dict keys), so it does not depend on the arena's layout; loads with
             ``torch.load(..., weights_only=True)``
  reference  what ``state_dict()`` of the inner ``torch.optim`` optimiser of the reference's ``get_optim`` (utils/optim.py:116-174)
             holds — ``RateOpt.__getattr__`` forwards ``state_dict`` to it, so the wrapper's ``_step`` is NOT in ``optimizer_last.pth``:
             per-parameter entries indexed in parameter order, one param group (dense) or two (supermask:
             scripts/train_n_prune_transformer.py:67-82)

Nothing here touches a device: the trainer hands over CPU tensors and gets CPU tensors back, and every refusal is raised from here,
before the trainer has written to an arena."""
import os
import warnings

import torch

FORMAT = 1
MASK_SUFFIX = "_pruning_mask"
# torch's own names of the arrays each kind keeps (ortk_optim_step's s1, s2 in this order)
STATE_ARRAYS = {"adam": ("exp_avg", "exp_avg_sq"), "sgd": (), "sgdm": ("momentum_buffer",), "sgdmom": ("momentum_buffer",),
                "rmsprop": ("square_avg",), "adagrad": ("sum",)}
STEPLESS = ("sgd", "sgdm", "sgdmom")          # torch.optim.SGD keeps no `step`
# OptimSpec fields: a difference in the first group refuses a native state, one in the second is listed in a warning
SPEC_MUST_MATCH = ("kind", "scheduler", "alpha", "beta", "eps", "weight_decay")
SPEC_INFO = ("d_model", "factor", "warmup", "max_train_step", "learning_rate", "learning_rate_min", "decay_start", "decay_every",
             "decay_rate")
# what the reference never switches on (its constructors leave torch's defaults): refused in a loaded param group
_UNSUPPORTED = {"amsgrad": False, "centered": False, "maximize": False, "lr_decay": 0, "initial_accumulator_value": 0}

# Registration order of the reference's modules (parameters() walks them in this order; the arena groups its entries differently).
# A parameter name sorts by the rank of each dotted component; a layer / head index sorts as a number.
_ORDER = ("att_embed", "model", "core", "encoder", "decoder", "src_embed", "tgt_embed", "generator", "layers", "self_attn", "src_attn",
          "feed_forward", "sublayer", "norm", "linears", "WGs", "w_1", "w_2", "lut", "proj", "weight", "bias", "a_2", "b_2")
_RANK = {n: i for i, n in enumerate(_ORDER)}


def _order_key(name):
    key = []
    for part in name.split("."):
        if part.isdigit():
            key.append(int(part))
        elif part in _RANK:
            key.append(_RANK[part])
        else:
            raise ValueError(f"parameter name {name!r}: component {part!r} has no place in the reference's module order")
    return key


def spec_fields(spec):
    return {k: getattr(spec, k) for k in SPEC_MUST_MATCH + SPEC_INFO}


def group_names(entries, supermask=False, frozen_scopes=None):
    """Parameter names per param group of the reference's optimiser, in its parameter order, from the arena's entry list (dicts with
    ``name`` and ``kind``: 0 plain, 1 maskable, 2 buffer).  Dense: [model.parameters()].  Supermask: [all_weights,
    active_pruning_masks] — the masks outside ``frozen_scopes`` (``prune_mask_freeze_scope``)."""
    names = sorted((e["name"] for e in entries if e["kind"] != 2), key=_order_key)
    if not supermask:
        return [names]
    maskable = {e["name"] for e in entries if e["kind"] == 1}
    frozen = tuple(frozen_scopes or ())
    masks = [n + MASK_SUFFIX for n in names if n in maskable and not any((n + MASK_SUFFIX).startswith(s) for s in frozen)]
    return [names, masks]


def build_torch_optimizer(spec, params):
    """The ``torch.optim`` instance ``get_optim`` builds for `spec` (utils/optim.py:116-174) over `params` (a list of parameters or
    of param-group dicts)."""
    from torch import optim
    lr, wd = spec.learning_rate, spec.weight_decay
    if spec.scheduler == "noam":
        return optim.Adam(params, lr=0, betas=(spec.alpha, spec.beta), eps=spec.eps)
    if spec.kind == "rmsprop":
        return optim.RMSprop(params, lr, spec.alpha, spec.eps, weight_decay=wd)
    if spec.kind == "adagrad":
        return optim.Adagrad(params, lr, weight_decay=wd)
    if spec.kind == "sgd":
        return optim.SGD(params, lr, weight_decay=wd)
    if spec.kind in ("sgdm", "sgdmom"):
        return optim.SGD(params, lr, spec.alpha, weight_decay=wd, nesterov=spec.kind == "sgdmom")
    if spec.kind == "adam":
        return optim.Adam(params, lr, (spec.alpha, spec.beta), spec.eps, weight_decay=wd)
    raise ValueError(f"Bad option `optim`: {spec.kind}")


def mask_group(params, mask_lr, mask_eps):
    """Second param group of scripts/train_n_prune_transformer.py:67-82."""
    return {"params": params, "lr": mask_lr, "weight_decay": 0, "eps": mask_eps, "pruning_mask": True}


def _entry_template(spec):
    """One per-parameter state entry as the installed torch writes it for this optimiser: a one-element parameter takes one step
    with a zero gradient.  Its keys, their order and the type of ``step`` are torch's, not restated here."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = build_torch_optimizer(spec, [p])
    p.grad = torch.zeros(1)
    opt.step()
    entry = opt.state_dict()["state"].get(0, {})
    arrays = set(entry) - {"step"}
    if arrays != set(STATE_ARRAYS[spec.kind]):
        raise RuntimeError(f"torch {torch.__version__} keeps {sorted(arrays)} for {spec.kind}, this package {STATE_ARRAYS[spec.kind]}")
    return entry


def _step_like(template, step):
    return template.new_tensor(step) if torch.is_tensor(template) else type(template)(step)


def pack_optimizer_state(spec, names, shapes, state=None, mask_state=None, optim_step=0, lr=None, mask_lr=100.0, mask_eps=1e-2):
    """The reference-format dict.  `names`: parameter names per group (``group_names``); `shapes`: name -> shape; `state` /
    `mask_state`: {array name: {parameter name: CPU fp32 tensor}} for group 0 / group 1, ``None`` = zeros; `lr`: the rate group 0
    last ran at (``None``: the constructor's)."""
    placeholders = [[torch.nn.Parameter(torch.empty(0)) for _ in g] for g in names]
    groups = placeholders[0] if len(names) == 1 else [{"params": placeholders[0]}, mask_group(placeholders[1], mask_lr, mask_eps)]
    out = build_torch_optimizer(spec, groups).state_dict()
    if lr is not None:
        out["param_groups"][0]["lr"] = lr
    template = _entry_template(spec)
    out["state"] = {}
    index = 0
    for g, source in zip(names, (state, mask_state)):
        for name in g:
            entry = {}
            for key, value in template.items():
                if key == "step":
                    entry[key] = _step_like(value, optim_step)
                elif source is None:
                    entry[key] = torch.zeros(tuple(shapes[name]))
                else:
                    entry[key] = source[key][name]
            if entry:
                out["state"][index] = entry
            index += 1
    return out


def _expected_constants(spec, masks, mask_lr, mask_eps):
    k = spec.kind
    c = {"weight_decay": 0 if masks else spec.weight_decay}
    if k == "adam":
        c.update(betas=(spec.alpha, spec.beta), eps=spec.eps)
    elif k in STEPLESS:
        c.update(momentum=0 if k == "sgd" else spec.alpha, nesterov=k == "sgdmom")
    elif k == "rmsprop":
        c.update(alpha=spec.alpha, eps=spec.eps, momentum=0)
    elif k == "adagrad":
        c.update(eps=spec.eps)
    if masks:
        c.update(lr=mask_lr, pruning_mask=True)
        if "eps" in c:
            c["eps"] = mask_eps
    return c


def unpack_optimizer_state(spec, d, names, shapes, mask_lr=100.0, mask_eps=1e-2):
    """Inverse of ``pack_optimizer_state`` with every check: returns (state, mask_state, step).  `step` is the entries' ``step`` as an
    int, or ``None`` where the kind stores none.  Raises ValueError on a group layout that does not fit `names`, on a constant that
    differs from `spec`, on an option the reference never uses, on a missing entry or array and on a shape mismatch."""
    groups = d.get("param_groups") if isinstance(d, dict) else None
    if not isinstance(groups, (list, tuple)) or "state" not in d:
        raise ValueError("not an optimiser state_dict: expected the keys `state` and `param_groups`")
    if len(groups) != len(names):
        raise ValueError(f"param group layout: the file has {len(groups)} group(s), this model's optimiser has {len(names)} "
                         "(dense: 1; supermask: weights and active pruning masks)")
    index = 0
    for gi, (g, gnames) in enumerate(zip(groups, names)):
        want = list(range(index, index + len(gnames)))
        if list(g.get("params", ())) != want:
            raise ValueError(f"param group {gi}: the file indexes {len(g.get('params', ()))} parameter(s) "
                             f"{list(g.get('params', ()))[:3]}..., this model has {len(gnames)} starting at {index}")
        index += len(gnames)
        for key, default in _UNSUPPORTED.items():
            if key in g and g[key] != default:
                raise ValueError(f"param group {gi}: {key} = {g[key]!r} is not supported (the reference runs with {default!r})")
        if bool(g.get("pruning_mask", False)) != (gi == 1):
            raise ValueError(f"param group {gi}: pruning_mask = {g.get('pruning_mask', False)!r}, expected {gi == 1}")
        for key, mine in _expected_constants(spec, gi == 1, mask_lr, mask_eps).items():
            theirs = g.get(key)
            if isinstance(mine, tuple):
                theirs = tuple(theirs) if isinstance(theirs, (list, tuple)) else theirs
            if theirs != mine:
                raise ValueError(f"param group {gi}: {key} is {theirs!r} in the file and {mine!r} in this trainer")
    arrays = STATE_ARRAYS[spec.kind]
    out = [{a: {} for a in arrays} for _ in names]
    steps = set()
    index = 0
    unknown = set(d["state"]) - set(range(sum(len(g) for g in names)))
    if unknown:
        raise ValueError(f"state entries for unknown parameter indices {sorted(unknown)[:5]}")
    for gi, gnames in enumerate(names):
        for name in gnames:
            entry = d["state"].get(index)
            index += 1
            if not arrays:
                continue
            if entry is None:
                raise ValueError(f"no state for parameter {name!r} (index {index - 1}) in the file")
            for a in arrays:
                if a not in entry or not torch.is_tensor(entry[a]):
                    raise ValueError(f"parameter {name!r}: the file has no `{a}` ({spec.kind} keeps {arrays}; it has {sorted(entry)})")
                if tuple(entry[a].shape) != tuple(shapes[name]):
                    raise ValueError(f"parameter {name!r}: `{a}` has shape {tuple(entry[a].shape)} in the file, {tuple(shapes[name])} here")
                out[gi][a][name] = entry[a].detach().to("cpu", torch.float32)
            if "step" in entry:
                steps.add(int(entry["step"]))
    if len(steps) > 1:
        raise ValueError(f"the entries carry different step counts {sorted(steps)}; the native trainer keeps one")
    step = steps.pop() if steps else None
    return out[0], (out[1] if len(names) > 1 else None), step


def resolve_steps(spec, step, rate_step):
    """(optim_step, rate step) after a reference-format load.  `step`: what ``unpack_optimizer_state`` found; `rate_step`: the caller's
    (``None`` = continue the schedule at the loaded step, 0 = the reference's resume)."""
    if rate_step is None and step is None:
        raise ValueError(f"rate_step: {spec.kind} stores no step count, so the schedule cannot be continued from the file; pass "
                         "rate_step (0 = the reference's resume)")
    if rate_step is not None and int(rate_step) < 0:
        raise ValueError(f"rate_step: {rate_step} is negative")
    # no `step` in the file: 1 = "a step has been taken" is all first_step asks (sgd keeps no state at all)
    optim_step = step if step is not None else int(len(STATE_ARRAYS[spec.kind]) > 0)
    return optim_step, (optim_step if rate_step is None else int(rate_step))


# ---------------------------------------------------------------------------------------------- native state
def check_native_state(sd, spec, names, shapes, mask_names, options):
    """Every refusal of ``NativeTrainer.load_state_dict``, off the device.  `names` / `mask_names`: the parameter names this trainer
    keeps state for (`mask_names` ``None``: no mask optimiser); `options`: its informational options.  Returns the list of
    informational differences (the caller warns once)."""
    if not isinstance(sd, dict) or sd.get("format") != FORMAT:
        raise ValueError(f"format: the state has {sd.get('format') if isinstance(sd, dict) else type(sd).__name__!r}, this trainer reads {FORMAT}")
    for key in ("rate_step", "optim_step", "epoch", "seed"):
        if key not in sd:
            raise ValueError(f"{key}: missing from the state (it has {sorted(sd)})")
    mine, saved = spec_fields(spec), sd.get("spec") or {}
    for key in SPEC_MUST_MATCH:
        if saved.get(key) != mine[key]:
            raise ValueError(f"{key}: the state was saved with {saved.get(key)!r}, this trainer runs {mine[key]!r}")
    if (sd.get("mask_state") is not None) != (mask_names is not None):
        raise ValueError(f"mask_state: the state {'has' if sd.get('mask_state') is not None else 'has no'} mask-optimiser arrays, this "
                         f"trainer {'trains' if mask_names is not None else 'does not train'} pruning masks (masked / dense mismatch)")
    arrays = STATE_ARRAYS[spec.kind]
    for field, want in (("state", names), ("mask_state", mask_names)):
        if want is None:
            continue
        maps = sd.get(field) or {}
        if sorted(maps) != sorted(arrays):
            raise ValueError(f"{field}: arrays {sorted(maps)} in the state, {sorted(arrays)} for {spec.kind}")
        for a in arrays:
            missing, unexpected = sorted(set(want) - set(maps[a])), sorted(set(maps[a]) - set(want))
            if missing or unexpected:
                raise ValueError(f"{field}.{a}: missing parameter(s) {missing[:4]}{'...' if len(missing) > 4 else ''}, unexpected "
                                 f"{unexpected[:4]}{'...' if len(unexpected) > 4 else ''} (state: {len(maps[a])} names, trainer: {len(want)})")
            for n in want:
                if tuple(maps[a][n].shape) != tuple(shapes[n]):
                    raise ValueError(f"{field}.{a}[{n!r}]: shape {tuple(maps[a][n].shape)} in the state, {tuple(shapes[n])} in this model")
    diff = [f"{k}: saved {saved.get(k)!r}, now {mine[k]!r}" for k in SPEC_INFO if saved.get(k) != mine[k]]
    diff += [f"{k}: saved {sd.get('options', {}).get(k)!r}, now {v!r}" for k, v in options.items() if sd.get("options", {}).get(k) != v]
    return diff


def warn_differences(diff):
    if diff:
        warnings.warn("the trainer's options differ from the saved ones (the trainer's hold): " + "; ".join(diff))


# ---------------------------------------------------------------------------------------------- files
def checkpoint_paths(log_dir, tag):
    """(model, optimizer, trainer): the first two are the reference's names (utils/training.py:82-83)."""
    return tuple(os.path.join(log_dir, f"{kind}_{tag}.pth") for kind in ("model", "optimizer", "trainer"))


def write_files(make_files):
    """Rank 0 writes ``make_files()`` = {path: object} — every file under a temporary name first, renamed once all are complete, so a
    killed process leaves the previous checkpoint whole — and the other ranks wait at a barrier."""
    from . import parallel
    if parallel.rank() == 0:
        done = []
        try:
            for path, obj in make_files().items():
                tmp = f"{path}.tmp{os.getpid()}"
                done.append((tmp, path))
                torch.save(obj, tmp)
            for tmp, path in done:
                os.replace(tmp, path)
        finally:
            for tmp, _ in done:
                if os.path.exists(tmp):
                    os.remove(tmp)
    parallel.barrier()


def read_file(path):
    return torch.load(path, map_location="cpu", weights_only=True)
