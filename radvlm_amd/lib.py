"""ctypes binding of libradvlm_hip.so (the C ABI declared in include/radvlm_hip.h).

The product path has no fallback: if the shared library is missing or a kernel returns an error code, this
module raises.  Tensors are plain torch CUDA(HIP) tensors used only as device memory; every call is
asynchronous on the current torch stream.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libradvlm_hip.so")

ACT_NONE, ACT_QUICK_GELU, ACT_GELU, ACT_GELU_TANH = 0, 1, 2, 3


class RadvlmHipError(RuntimeError):
    pass


_HEADER = os.path.join(os.path.dirname(_HERE), "include", "radvlm_hip.h")
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}
_DECL = re.compile(r"(.+?)\b(rv_\w+)\s*\((.*)\)", re.S)
_PARAM = re.compile(r"(const\s+)?(\w+)(\s*\*\s*|\s+)(\w+)")


def _ctype(base, pointer, what):
    if pointer:
        return ctypes.c_void_p
    if base not in _SCALARS:
        raise RadvlmHipError(f"radvlm_hip.h: {what}: no ctypes type for '{base}'")
    return _SCALARS[base]


def parse_header(text):
    """{name: (restype, argtypes)} of every rv_* declaration in the C text of a header.  One fixed type map (any pointer is a
    c_void_p, a `const char*` return a c_char_p, the scalars of _SCALARS); anything else raises, naming the function and the parameter."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:.*\\\n)*.*$", " ", text, flags=re.M)
    sigs = {}
    for stmt in text.split(";"):
        stmt = re.split(r"[{}]", stmt)[-1].strip()             # what follows `extern "C" {`
        if "rv_" not in stmt:
            continue
        m = _DECL.fullmatch(stmt)
        if not m:
            raise RadvlmHipError(f"radvlm_hip.h: cannot parse the declaration '{' '.join(stmt.split())}'")
        ret, name, params = " ".join(m.group(1).split()), m.group(2), [" ".join(p.split()) for p in m.group(3).split(",")]
        r = re.fullmatch(r"(const )?(\w+) ?(\*)?", ret)
        if not r:
            raise RadvlmHipError(f"radvlm_hip.h: {name}: cannot parse the return type '{ret}'")
        restype = ctypes.c_char_p if ret == "const char*" else _ctype(r.group(2), r.group(3), f"{name}: return type")
        argtypes = []
        for p in ([] if params == ["void"] else params):
            q = _PARAM.fullmatch(p)
            if not q:
                raise RadvlmHipError(f"radvlm_hip.h: {name}: cannot parse the parameter '{p}' (a type and a name are required)")
            argtypes.append(_ctype(q.group(2), "*" in q.group(3), f"{name}: parameter '{p}'"))
        if name in sigs:
            raise RadvlmHipError(f"radvlm_hip.h: {name} is declared twice")
        sigs[name] = (restype, argtypes)
    return sigs


def _read_header():
    if not os.path.exists(_HEADER):
        raise RadvlmHipError(f"{_HEADER} not found: the ctypes signatures are derived from it")
    with open(_HEADER) as f:
        return parse_header(f.read())


SIGNATURES = _read_header()             # the header is the one place an entry point is declared: name -> (restype, argtypes)
EXPORTED_SYMBOLS = sorted(SIGNATURES)

_lib = None


def bind(path):
    """Open a build of the library and type every declared entry point (the product build, or a second one for an A/B tool)."""
    if not os.path.exists(path):
        raise RadvlmHipError(f"{path} not found: build it with radvlm_amd/csrc/build.sh "
                             "(or __graft_entry__.build()); there is no CPU fallback")
    lib = ctypes.CDLL(path)
    missing = [name for name in SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise RadvlmHipError(f"{path} lacks symbols of radvlm_hip.h: {missing}")
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def load():
    """Load the shared library (no GPU needed to load); raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = bind(os.environ.get("RADVLM_HIP_LIB", _LIB_PATH))     # override: A/B of two builds (tools/), never a fallback
    return _lib


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, int):
        return t
    assert t.is_cuda, "radvlm_amd kernels take device tensors only"
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*[(_ptr(a) if (a is None or isinstance(a, torch.Tensor)) else a) for a in args], _stream())
    if rc != 0:
        raise RadvlmHipError(f"{name} failed with code {rc}")


_zeros = {}


def zeros16(device=None):
    device = torch.device(device or torch.cuda.current_device())
    key = (device.type, device.index)
    if key not in _zeros:
        _zeros[key] = torch.zeros(64, dtype=torch.uint8, device=device)
    return _zeros[key]
