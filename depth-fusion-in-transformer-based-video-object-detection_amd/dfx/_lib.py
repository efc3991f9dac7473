"""ctypes loader of libdfx.so.  The C ABI is read from include/*.h: every ``dfx_*`` prototype gives the argument and return
types of its entry point (0 = ok, <0 = DFX_E* for the int ones), every ``#define DFX_<NAME> <integer>`` a constant."""
import ctypes
import glob
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# DFX_LIBRARY selects another build of the library (diagnostic / ablation builds of tools/ab.sh); it must exist - there is no
# fall back to the shipped one
_SO = os.environ.get("DFX_LIBRARY") or os.path.join(_HERE, "libdfx.so")
_lib = None

# <package>/../../include: the directory csrc/Makefile compiles the library against
_INCLUDE = os.path.normpath(os.path.join(_HERE, "..", "..", "include"))
_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}
_PROTOTYPE = re.compile(r"\b(int|const\s+char\s*\*)\s*(dfx_\w+)\s*\(([^()]*)\)\s*;")
# object-like macros with a value: an include guard has none, a function-like macro has its "(" right behind the name
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(DFX_\w+)[ \t]+(\S.*?)[ \t]*$", re.M)
_INT_PRODUCT = re.compile(r"-?\d+(?:\s*\*\s*\d+)*")


def parse_header(text):
    """The C ABI one header declares -> ({function: (restype, argtypes)}, {DFX_NAME: int}).  A scalar parameter type or a
    macro value outside the forms below raises by name: a guessed type hands a kernel garbage strides."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).replace("\\\n", " ")
    prototypes, constants = {}, {}
    for ret, name, params in _PROTOTYPE.findall(text):
        argtypes = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            words = [w for w in param.split() if w != "const"]
            ctype = ctypes.c_void_p if "*" in param else _SCALARS.get(" ".join(words[:-1]))
            if ctype is None:
                raise RuntimeError(f"{name}: parameter '{param.strip()}' is not a pointer, int, long, float or double")
            argtypes.append(ctype)
        prototypes[name] = (ctypes.c_int if ret == "int" else ctypes.c_char_p, argtypes)
    for name, expr in _DEFINE.findall(text):
        inner = expr[1:-1].strip() if expr.startswith("(") and expr.endswith(")") else expr
        if not _INT_PRODUCT.fullmatch(inner):
            raise RuntimeError(f"#define {name} {expr}: not an integer or a product of integers")
        value = 1
        for factor in inner.split("*"):
            value *= int(factor)
        constants[name] = value
    return prototypes, constants


def _parse_headers():
    headers = sorted(glob.glob(os.path.join(_INCLUDE, "*.h")))
    if not headers:
        raise RuntimeError(f"{_INCLUDE} holds no headers: the C ABI of libdfx.so is read from include/*.h of the source "
                           "tree, which must sit next to the package as it does in the repository.")
    prototypes, constants = {}, {}
    for h in headers:
        with open(h) as f:
            p, c = parse_header(f.read())
        prototypes.update(p)
        constants.update(c)
    return prototypes, constants


_PROTOTYPES, CONSTANTS = _parse_headers()      # CONSTANTS: every `#define DFX_<NAME> <integer>` of the headers
SIGNATURES = {name: argtypes for name, (_, argtypes) in _PROTOTYPES.items()}      # name -> argtypes
ENONFINITE = CONSTANTS["DFX_ENONFINITE"]


class LevelLayout(ctypes.Structure):
    """dfx_msda_level_layout (include/dfx_msda.h): operand strides of the level-in-LDS kernel, in floats."""
    _fields_ = [(n, ctypes.c_long) for n in (
        "value_frame", "value_token", "value_head", "value_oct", "value_chunk",
        "off_row", "off_head", "logit_row", "logit_head",
        "out_row", "out_head", "out_oct", "out_chunk")]


def library_path():
    return _SO


def load():
    """Return the loaded library; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise RuntimeError(
                f"{_SO} is missing: the HIP extension has not been built "
                "(run `python __graft_entry__.py build` or `make -C <pkg>/csrc`). "
                "There is no CPU or PyTorch fallback for this operator.")
        lib = ctypes.CDLL(_SO)
        for name, (restype, argtypes) in _PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, restype
        _lib = lib
    return _lib


def abi_version():
    return load().dfx_abi_version()


def check(rc, what):
    if rc != 0:
        msg = load().dfx_last_error().decode() or f"error code {rc}"
        raise RuntimeError(f"{what}: {msg}")
