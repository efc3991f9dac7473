"""Weight-update lifecycle: one tensor of a model changes after the fused inference routes have run (and have cached what
they derive from the weights - folded BN, transformed filters, stacked projections: models.fused.derived_key), and the next
run must give what a module that has never run gives with the same weights.  Bit for bit: same kernels, same data.

An edit kind is a function ``(owner_module, tensor_name) -> None`` that changes exactly that tensor, the way user code does:

  inplace       with no_grad(): t.mul_(1.25).add_(0.01)              (bumps t._version)
  optimizer     t.grad = seeded randn; SGD([t], lr=0.05).step()      (bumps t._version; parameters only)
  load          owner.load_state_dict({name: new}, strict=False)     (in-place copy: bumps t._version)
  assign        the same with assign=True                            (a new Parameter object / a new buffer tensor)
  replace       t.data = new  /  setattr(owner, name, new) for a buffer   (new storage, the version counter stays)
  data_inplace  t.data.mul_(1.25)                                    (neither moves: assert_follows then calls drop_derived)

(x 1.25 + 0.01 keeps a running variance positive and moves a zero tensor.)
"""
import re

import torch

PARAM_KINDS = ("inplace", "replace")
BUFFER_KINDS = ("inplace", "replace")
EXTRA_KINDS = ("optimizer", "load", "assign", "data_inplace")          # for one representative tensor of every site

# Tensors that cannot change an output, by name pattern, each with its reason.  Nothing else is left out: ``sources`` asserts it.
EXCLUDED = (
    (r"(^|\.)fc\.(weight|bias)$", "the ImageNet classifier of the ResNet: kept for checkpoint keys, never called by a detector"),
    (r"(^|\.)num_batches_tracked$", "an integer step counter of nn.BatchNorm2d: no arithmetic reads it in eval mode"),
    (r"(^|\.)downsample_layers_e\.3\.", "the fourth DFormer depth stage: DFormerBackbone.forward never runs it"),
)


def _new_value(t):
    return (t.detach() * 1.25 + 0.01).clone()


def _is_buffer(owner, name):
    return name in owner._buffers


def inplace(owner, name):
    with torch.no_grad():
        getattr(owner, name).mul_(1.25).add_(0.01)


def optimizer(owner, name):
    t = getattr(owner, name)
    assert isinstance(t, torch.nn.Parameter), "the optimizer kind is for parameters"
    t.grad = torch.randn(t.shape, generator=torch.Generator().manual_seed(17)).to(device=t.device, dtype=t.dtype)
    torch.optim.SGD([t], lr=0.05).step()
    t.grad = None


def _load(owner, name, assign):
    res = owner.load_state_dict({name: _new_value(getattr(owner, name))}, strict=False, assign=assign)
    assert name not in res.missing_keys and not res.unexpected_keys


def load(owner, name):
    _load(owner, name, False)


def assign(owner, name):
    before = getattr(owner, name)
    _load(owner, name, True)
    assert getattr(owner, name) is not before, "load_state_dict(assign=True) is expected to install a new tensor object"


def replace(owner, name):
    t = getattr(owner, name)
    if _is_buffer(owner, name):
        setattr(owner, name, _new_value(t))
    else:
        t.data = _new_value(t)


def data_inplace(owner, name):
    getattr(owner, name).data.mul_(1.25)


EDITS = {f.__name__: f for f in (inplace, optimizer, load, assign, replace, data_inplace)}


def sources(module, only=None):
    """Every floating tensor of ``module`` that can reach an output: [(owner_path, tensor_name, is_buffer)], parameters and
    buffers, each once, minus EXCLUDED - and an assertion that nothing else is missing.  ``only``: a predicate on the dotted
    name, for a site that is a part of ``module`` (the assertion then covers that part)."""
    out, left_out, seen = [], [], set()
    for path, mod in module.named_modules():
        for table, is_buffer in ((mod._parameters, False), (mod._buffers, True)):
            for name, t in table.items():
                full = f"{path}.{name}" if path else name
                if t is None or id(t) in seen or (only is not None and not only(full)):
                    continue
                seen.add(id(t))
                if any(re.search(pat, full) for pat, _ in EXCLUDED):
                    left_out.append(full)
                elif t.is_floating_point():
                    out.append((path, name, is_buffer))
                else:
                    raise AssertionError(f"{full}: an integer tensor that no exclusion names")
    want = {n for n, t in list(module.named_parameters()) + list(module.named_buffers())
            if t.is_floating_point() and (only is None or only(n))}
    got = {f"{p}.{n}" if p else n for p, n, _ in out}
    assert got | {n for n in left_out if n in want} == want, sorted(want - got)
    return out


def case_list(srcs, representative):
    """[(owner_path, tensor_name, kind)] for pytest.mark.parametrize: the two basic kinds for every source tensor, the four
    further kinds for ``representative`` = (owner_path, tensor_name) (``optimizer`` only where it is a parameter)."""
    cases = []
    for path, name, is_buffer in srcs:
        cases += [(path, name, k) for k in (BUFFER_KINDS if is_buffer else PARAM_KINDS)]
        if (path, name) == tuple(representative):
            cases += [(path, name, k) for k in EXTRA_KINDS if not (is_buffer and k == "optimizer")]
    assert any((p, n) == tuple(representative) for p, n, _ in srcs), representative
    return cases


def case_id(case):
    path, name, kind = case
    return f"{path + '.' if path else ''}{name}-{kind}"


def tensors_of(y):
    """The tensors of a run's result (a tensor, or nested lists / tuples / dicts / NestedTensors of them), in a fixed order."""
    if torch.is_tensor(y):
        return [y]
    if isinstance(y, dict):
        return [t for k in sorted(y) for t in tensors_of(y[k])]
    if isinstance(y, (list, tuple)):
        return [t for v in y for t in tensors_of(v)]
    if hasattr(y, "tensors") and hasattr(y, "mask"):
        return [y.tensors]
    return []


def assert_same(got, want, what):
    got, want = tensors_of(got), tensors_of(want)
    assert len(got) == len(want) and len(got) > 0, what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(a, b), \
            f"{what}: output {i} differs in {(a != b).sum().item()} of {a.numel()} elements, max {(a.double() - b.double()).abs().max().item():.3e}"


def differs(a, b):
    return any(x.shape != y.shape or not torch.equal(x, y) for x, y in zip(tensors_of(a), tensors_of(b)))


def run_twice(run, model):
    """-> the result of two equal runs under no_grad (the second one meets every cache), asserted bit-equal."""
    with torch.no_grad():
        first = [t.clone() for t in tensors_of(run(model))]
        second = [t.clone() for t in tensors_of(run(model))]
    assert_same(second, first, "two runs with nothing in between")
    return second


def fresh_reference(build, run, model):
    """What a module that has never run gives with ``model``'s current state."""
    b = build()
    b.load_state_dict(model.state_dict())
    with torch.no_grad():
        return [t.clone() for t in tensors_of(run(b))]


def apply_edit(model, owner_path, tensor_name, kind, runner=None):
    owner = model.get_submodule(owner_path) if owner_path else model
    EDITS[kind](owner, tensor_name)
    if kind == "data_inplace":              # no key can see this one (models.fused.derived_key): the caller says so
        from models.fused import drop_derived
        assert drop_derived(model) > 0
        if runner is not None:
            runner.refresh()


def assert_follows(build, run, owner_path, tensor_name, kind, after_first_runs=None):
    """``build()`` -> a seeded model on the GPU in eval mode with fused inference on; ``run(model)`` -> its outputs.
    after_first_runs(model): the case's own assertions about the route the first runs took."""
    from util import memo
    memo.clear()           # entries are keyed on a tensor's address and version: an earlier case's freed model may have had both
    a = build()
    y0 = run_twice(run, a)
    if after_first_runs is not None:
        after_first_runs(a)
    apply_edit(a, owner_path, tensor_name, kind)
    with torch.no_grad():
        y1 = [t.clone() for t in tensors_of(run(a))]
    y_ref = fresh_reference(build, run, a)
    assert_same(y1, y_ref, f"{kind} of {owner_path}.{tensor_name}: the module that had run before the edit against a fresh one")
    assert differs(y1, y0), f"{kind} of {owner_path}.{tensor_name} did not change any output: the case checks nothing"
