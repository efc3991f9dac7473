"""INTEGRATION.md path A: a caller laid out as the reference's ``models/ops/functions/ms_deform_attn_func.py`` and
``models/ops/modules/ms_deform_attn.py`` - ``import MultiScaleDeformableAttention as MSDA`` where the reference imports its
compiled pybind11 module (ms_deform_attn_func.py:18-38 of the reference) - gets this repository's
``MultiScaleDeformableAttention.py`` (the ctypes shim over libdfx.so) from nothing but the package directory on the path: the
module resolves to the shim, both entry points are found with the header's parameter lists (ms_deform_attn.h:20-38,41-61), and
CPU tensors raise the reference's "Not implemented on the CPU" through the autograd Function and through the MSDeformAttn
module.  The callers are the package's own two files of that layout, imported the way the reference's are (a namespace
``models`` package, so nothing else of the package is loaded); the reference itself is not part of this repository.  (On a
GPU the same import runs the HIP kernels; the numerics of that path are tests/test_msda_gpu.py's.)

Runs in a subprocess: only the package directory may be on the path, as for a caller outside this repository.
"""
import os
import subprocess
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "depth-fusion-in-transformer-based-video-object-detection_amd")

SCRIPT = r"""
import inspect, os, sys, types
PKG = sys.argv[1]
# what `PYTHONPATH=<PKG> python <caller>` gives a caller outside this repository
sys.path[:0] = [PKG]
pkg = types.ModuleType("models")            # a namespace import: only the two files below are loaded
pkg.__path__ = [PKG + "/models"]
sys.modules["models"] = pkg
import torch
import models.ops.functions.ms_deform_attn_func as f          # `import MultiScaleDeformableAttention as MSDA`, as the reference's
from models.ops.modules import MSDeformAttn
assert f.__file__.startswith(PKG) and inspect.getfile(MSDeformAttn).startswith(PKG)
assert f.MSDA.__file__ == os.path.join(PKG, "MultiScaleDeformableAttention.py"), f.MSDA.__file__
fwd, bwd = f.MSDA.ms_deform_attn_forward, f.MSDA.ms_deform_attn_backward
assert list(inspect.signature(fwd).parameters) == ["value", "spatial_shapes", "level_start_index", "sampling_loc", "attn_weight", "im2col_step"]
assert list(inspect.signature(bwd).parameters) == ["value", "spatial_shapes", "level_start_index", "sampling_loc", "attn_weight", "grad_output", "im2col_step"]
v = torch.zeros(1, 4, 8, 32); s = torch.tensor([[2, 2]]); l = torch.tensor([0])
loc = torch.zeros(1, 3, 8, 1, 4, 2); aw = torch.zeros(1, 3, 8, 1, 4)
for call in (lambda: f.MSDeformAttnFunction.apply(v, s, l, loc, aw, 64),
             lambda: bwd(v, s, l, loc, aw, torch.zeros(1, 3, 256), 64),
             lambda: MSDeformAttn(256, 1, 8, 4)(torch.zeros(1, 3, 256), torch.rand(1, 3, 1, 2), torch.zeros(1, 4, 256), s, l)):
    try:
        call()
    except RuntimeError as e:
        assert "Not implemented on the CPU" in str(e), str(e)
    else:
        raise AssertionError("CPU tensors must be refused")
print("PATH_A_OK")
"""


def test_reference_modules_import_the_shim_unchanged():
    out = subprocess.run([sys.executable, "-c", SCRIPT, PKG], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "PATH_A_OK" in out.stdout, out.stderr[-2000:]
