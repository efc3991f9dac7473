"""AdamW with norm clipping on the table kernels of include/dfx_optim.h (csrc/optim.hip): the tail of the reference's
training iteration, ``clip_grad_norm_(model.parameters(), max_norm)`` + ``optimizer.step()`` (ref engine_single.py:61-67,
engine_multi.py:64), as two launches over all parameters instead of a chain of ``_foreach_*`` calls.

    opt = dfx.optim.AdamW(param_groups, lr=2e-4, weight_decay=1e-4)
    loss.backward()
    norm = opt.step(max_norm=0.1)            # a 0-dim device tensor; nothing waits for the GPU

Per step the host writes one record per parameter that has a gradient (its four pointers, its size, the scalars of this
step computed in double from the parameter's own ``step`` as torch.optim.adamw computes them) and one record per
``CHUNK`` elements into pinned memory, uploads both with one asynchronous copy on the current stream and launches.
There is no CPU implementation: a parameter that is not on the GPU is refused at construction.
"""
import numpy as np
import torch

from . import _lib
from .ops import _call

# dfx_optim_tensor / dfx_optim_chunk of include/dfx_optim.h
_TENSOR = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("numel", "<i8"),
                    ("scalars", "<f4", (7,)), ("reserved", "<f4")])
_CHUNK = np.dtype([("first", "<i8"), ("tensor", "<i4"), ("reserved", "<i4")])
assert _TENSOR.itemsize == 72 and _CHUNK.itemsize == 16

_chunk_elements = None


def chunk_elements():
    """DFX_OPTIM_CHUNK of the loaded library: elements per chunk record."""
    global _chunk_elements
    if _chunk_elements is None:
        _chunk_elements = int(_lib.load().dfx_optim_chunk_elements())
    return _chunk_elements


def _chunk_table(numels):
    """one record per CHUNK elements of every tensor, tensor after tensor; none for an empty tensor"""
    chunk = chunk_elements()
    counts = (np.asarray(numels, dtype=np.int64) + (chunk - 1)) // chunk
    table = np.zeros(int(counts.sum()), dtype=_CHUNK)
    table["tensor"] = np.repeat(np.arange(len(numels), dtype=np.int32), counts)
    starts = np.cumsum(counts) - counts
    table["first"] = (np.arange(len(table), dtype=np.int64) - np.repeat(starts, counts)) * chunk
    return table


class _Staging:
    """Pinned upload buffers.  A buffer is written again only after the copy that last read it has completed (its event
    says so without waiting); while none is free a new one is made, so a step never waits for an earlier one."""

    def __init__(self):
        self.slots = []          # [pinned uint8 tensor, event recorded behind its last copy]

    def upload(self, device, tensors, chunks):
        """-> (device uint8 tensor holding both tables, byte offset of the chunk table)"""
        off = (tensors.nbytes + 15) & ~15
        total = off + chunks.nbytes
        slot = None
        for s in self.slots:
            if s[0].numel() >= total and s[1].query():
                slot = s
                break
        if slot is None:
            self.slots = [s for s in self.slots if s[0].numel() >= total or not s[1].query()]     # outgrown and idle: dropped
            slot = [torch.empty((max(total, 1) + 4095) & ~4095, dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
            self.slots.append(slot)
        host = slot[0].numpy()
        host[:tensors.nbytes] = tensors.view(np.uint8).reshape(-1)
        host[off:total] = chunks.view(np.uint8).reshape(-1)
        dev = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
        dev[:total].copy_(slot[0][:total], non_blocking=True)
        slot[1].record(torch.cuda.current_stream(device))
        return dev, off


def _check_grad(i, p, g, device):
    if g.is_sparse or g.layout != torch.strided:
        raise RuntimeError(f"dfx.optim: the gradient of parameter {i} is sparse")
    if not g.is_contiguous():
        raise RuntimeError(f"dfx.optim: the gradient of parameter {i} is not contiguous")
    if g.dtype != torch.float32 or g.device != device or g.shape != p.shape:
        raise RuntimeError(f"dfx.optim: the gradient of parameter {i} is {g.dtype} {tuple(g.shape)} on {g.device}, "
                           f"expected torch.float32 {tuple(p.shape)} on {device}")


_norm_staging = {}


@torch.no_grad()
def grad_norm(parameters):
    """The 2-norm of all gradients of ``parameters`` as a 0-dim fp32 device tensor (what the reference's
    ``utils.get_total_grad_norm`` reports when max_norm is 0): the norm kernel alone (dfx_grad_sqnorm_f32: squares and
    per-chunk sums in fp64), its partials added by torch in fp64 and rounded to fp32 once.  Parameters without a gradient are
    skipped; nothing waits for the GPU."""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        raise ValueError("dfx.optim.grad_norm: no parameter has a gradient")
    device = params[0].grad.device
    if device.type != "cuda":
        raise RuntimeError("Not implemented on the CPU (dfx.optim.grad_norm needs gradients on the GPU)")
    for i, p in enumerate(params):
        _check_grad(i, p, p.grad, device)
    rec = np.zeros(len(params), dtype=_TENSOR)
    rec["grad"] = [p.grad.data_ptr() for p in params]
    rec["numel"] = [p.numel() for p in params]
    chunks = _chunk_table(rec["numel"])
    n = len(chunks)
    if n == 0:
        return torch.zeros((), dtype=torch.float32, device=device)
    tables, off = _norm_staging.setdefault(device, _Staging()).upload(device, rec, chunks)
    partials = torch.empty(n, dtype=torch.float64, device=device)
    _call("grad_norm", "dfx_grad_sqnorm_f32", device, tables.data_ptr(), tables.data_ptr() + off, n, partials.data_ptr())
    return partials.sum().sqrt().float()


class AdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` (fp32, no amsgrad) whose ``step`` is one HIP launch over all parameters, two with clipping.

    Same constructor, parameter groups, hyper-parameter keys and state (``step`` a CPU fp32 tensor, ``exp_avg``,
    ``exp_avg_sq``) as torch's class: ``state_dict()`` / ``load_state_dict()`` interchange with it in both directions and
    lr schedulers drive it through ``param_groups``.  Parameters are contiguous fp32 tensors on one GPU.

    ``step(max_norm=m)`` with m > 0 is ``clip_grad_norm_(all parameters of the optimizer, m)`` followed by ``step()`` and
    returns the total norm (a 0-dim fp32 device tensor).  One difference: the clipped gradient is used, not stored -
    ``.grad`` holds the UNSCALED gradient afterwards, where clip_grad_norm_ leaves the scaled one (the reference's loop
    never reads gradients after the step).  The norm is summed in fp64 and rounded once, torch's in fp32.
    Non-finite values get no special handling, as in torch: one infinite gradient gives the coefficient 0, NaN in that
    element and a zero gradient in all others.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False, capturable=False, differentiable=False):
        for name, val in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable), ("differentiable", differentiable)):
            if val:
                raise ValueError(f"dfx.optim.AdamW does not implement {name}=True")
        # the keys of torch.optim.AdamW's groups, so that either class loads the other's state_dict
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        self._device = None
        self._n_seen = 0
        self._layout = None          # (ids, numels, chunk table) of the parameters of the last step
        self._staging = _Staging()
        super().__init__(params, defaults)

    @staticmethod
    def _check_group(group):
        lr, (beta1, beta2) = group["lr"], group["betas"]
        if torch.is_tensor(lr) or torch.is_tensor(beta1) or torch.is_tensor(beta2):
            raise ValueError("dfx.optim.AdamW: lr and betas are Python numbers (tensor hyper-parameters belong to capturable=True)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= group["eps"]:
            raise ValueError(f"Invalid epsilon value: {group['eps']}")
        if not 0.0 <= beta1 < 1.0 or not 0.0 <= beta2 < 1.0:
            raise ValueError(f"Invalid beta parameters: {group['betas']}")
        if not 0.0 <= group["weight_decay"]:
            raise ValueError(f"Invalid weight_decay value: {group['weight_decay']}")
        for name in ("amsgrad", "maximize", "capturable", "differentiable", "fused"):
            if group.get(name):
                raise ValueError(f"dfx.optim.AdamW does not implement {name}=True")
        if group.get("decoupled_weight_decay") is False:
            raise ValueError("dfx.optim.AdamW decays the weights decoupled from the gradient (AdamW, not Adam)")

    def add_param_group(self, param_group):
        before = len(self.param_groups)
        super().add_param_group(param_group)
        if len(self.param_groups) == before:
            return
        group = self.param_groups[-1]
        try:
            self._check_group(group)
            for p in group["params"]:
                i = self._n_seen
                if not p.is_cuda:
                    raise ValueError(f"dfx.optim.AdamW: parameter {i} is on {p.device}: Not implemented on the CPU")
                if p.dtype != torch.float32:
                    raise ValueError(f"dfx.optim.AdamW: parameter {i} is {p.dtype}, expected torch.float32")
                if p.layout != torch.strided or not p.is_contiguous():
                    raise ValueError(f"dfx.optim.AdamW: parameter {i} is not contiguous")
                if self._device is None:
                    self._device = p.device
                if p.device != self._device:
                    raise ValueError(f"dfx.optim.AdamW: parameter {i} is on {p.device}, the ones before it on {self._device}")
                self._n_seen += 1
        except ValueError:
            self.param_groups.pop()
            raise
        self._layout = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)
        self._layout = None

    def _init_state(self, p):
        state = self.state[p]
        state["step"] = torch.tensor(0.0, dtype=torch.float32)
        state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    def _host_tables(self):
        """Advance ``step`` of every parameter that has a gradient (making its state on first sight) and -> (params, tensor
        records, chunk records) of this step in host memory, or None when no parameter has a gradient."""
        device = self._device
        params, grads, states, group_of = [], [], [], []
        i = 0
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    if g.is_sparse or g.dtype != torch.float32 or g.device != device or not g.is_contiguous():
                        _check_grad(i, p, g, device)
                    state = self.state[p]
                    if len(state) == 0:
                        state = self._init_state(p)
                    params.append(p), grads.append(g), states.append(state), group_of.append(gi)
                i += 1
        if not params:
            return None
        ids, numels = [id(p) for p in params], [p.numel() for p in params]
        if self._layout is None or self._layout[0] != ids or self._layout[1] != numels:
            for p, g, s in zip(params, grads, states):
                for name in ("exp_avg", "exp_avg_sq"):
                    t = s[name]
                    if t.dtype != torch.float32 or t.device != device or t.shape != p.shape or not t.is_contiguous():
                        raise RuntimeError(f"dfx.optim.AdamW: state {name} must be a contiguous fp32 tensor of the parameter's shape on {device}")
                if s["step"].is_cuda:
                    raise RuntimeError("dfx.optim.AdamW: the step counters live on the CPU (this state comes from capturable / fused torch)")
                if not p.is_contiguous() or g.shape != p.shape:
                    raise RuntimeError("dfx.optim.AdamW: a parameter is no longer contiguous, or its gradient has another shape")
            self._layout = (ids, numels, _chunk_table(numels))
        chunks = self._layout[2]

        steps = [s["step"] for s in states]
        torch._foreach_add_(steps, 1.0)
        step_values = torch.stack(steps).tolist()
        scalars, memo = [], {}
        for gi, step in zip(group_of, step_values):
            row = memo.get((gi, step))
            if row is None:
                group = self.param_groups[gi]
                lr, (beta1, beta2), wd = group["lr"], group["betas"], group["weight_decay"]
                bias_correction1 = 1 - beta1 ** step
                bias_correction2 = 1 - beta2 ** step
                row = memo[(gi, step)] = (1 - lr * wd, 1 - beta1, beta2, 1 - beta2, lr / bias_correction1,
                                          bias_correction2 ** 0.5, group["eps"])
            scalars.append(row)
        rec = np.zeros(len(params), dtype=_TENSOR)
        rec["param"] = [p.data_ptr() for p in params]
        rec["grad"] = [g.data_ptr() for g in grads]
        rec["exp_avg"] = [s["exp_avg"].data_ptr() for s in states]
        rec["exp_avg_sq"] = [s["exp_avg_sq"].data_ptr() for s in states]
        rec["numel"] = numels
        rec["scalars"] = np.asarray(scalars, dtype=np.float64)          # rounded to fp32 once, here
        return params, rec, chunks

    @torch.no_grad()
    def step(self, closure=None, max_norm=0.0):
        """One AdamW step of every parameter that has a gradient; -> the total gradient norm (0-dim fp32 device tensor) when
        ``max_norm > 0`` - the gradients are then clipped to it as by clip_grad_norm_, but ``.grad`` is left unscaled - else
        None.  A parameter whose ``.grad`` is None is skipped: no state is made, its ``step`` and version stay.  ``closure``
        is called for its gradients; its value is not returned.  Enqueues on the current stream and returns."""
        if closure is not None:
            with torch.enable_grad():
                closure()
        host = self._host_tables()
        if host is None:
            return None
        params, rec, chunks = host
        device = self._device
        n = len(chunks)
        norm = None
        if n > 0:
            tables, off = self._staging.upload(device, rec, chunks)
            tp, cp = tables.data_ptr(), tables.data_ptr() + off
            if max_norm > 0:
                partials = torch.empty(n, dtype=torch.float64, device=device)
                norm = torch.empty((), dtype=torch.float32, device=device)
                _call("AdamW.step", "dfx_grad_sqnorm_f32", device, tp, cp, n, partials.data_ptr())
                _call("AdamW.step", "dfx_adamw_step_f32", device, tp, cp, n, partials.data_ptr(), float(max_norm), norm.data_ptr())
            else:
                _call("AdamW.step", "dfx_adamw_step_f32", device, tp, cp, n, None, 0.0, None)
        elif max_norm > 0:
            norm = torch.zeros((), dtype=torch.float32, device=device)
        # the kernel wrote the parameters behind autograd's back: move their version counters, so that every route that
        # cached something derived from them (models.fused.derived_key) rebuilds it
        torch.autograd.graph.increment_version(params)
        return norm
