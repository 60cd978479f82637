"""ctypes binding of ``libctvae_hip.so`` (C ABI: ``include/ctvae_hip.h``).

The product path has NO CPU or eager-PyTorch fallback: if the library is missing, cannot be loaded or
a launch fails, a ``RuntimeError`` is raised (SURVEY.md §8b "Errors").  Tensors are passed as raw device
pointers; the current torch stream is passed as the ``hipStream_t``.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CTVAE_LIB_OVERRIDE") or os.path.join(_HERE, "lib", "libctvae_hip.so")   # override: A/B of two builds in one gpurun call
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ctvae_hip.h")

_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
            "double": ctypes.c_double}
_TYPE_WORDS = set(_SCALARS) | {"void", "char", "short", "unsigned", "signed"}   # never a parameter's name


def _ctype(decl: str, proto: str, named: bool):
    """ctypes type of one parameter declaration (`named`: it ends in the parameter's name) or of a return type."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        return ctypes.c_char_p if words[0] == "char" else ctypes.c_void_p
    if named and len(words) > 1 and words[-1] not in _TYPE_WORDS:
        words.pop()
    t = " ".join(words)
    if t == "void" and not named:
        return None
    if t not in _SCALARS:
        raise RuntimeError(f"ctvae_hip.h: no ctypes type for '{' '.join(decl.split())}' in: {proto}")
    return _SCALARS[t]


def parse_prototypes(text: str) -> dict:
    """{name: (restype, argtypes, has_stream)} of every `<return type> ctvae_name(<params>);` in a C header's text."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s*]*?)\b(ctvae_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        proto = " ".join(m.group(0).split())
        params = [p for p in m.group(3).split(",") if p.split() not in ([], ["void"])]
        has_stream = bool(params) and params[-1].replace("*", " * ").split() == ["void", "*", "stream"]
        out[m.group(2)] = (_ctype(m.group(1), proto, False), [_ctype(p, proto, True) for p in params], has_stream)
    return out


if not os.path.exists(HEADER_PATH):
    raise RuntimeError(f"{HEADER_PATH} is missing: the ctypes signatures of libctvae_hip.so are read from it")
with open(HEADER_PATH) as _f:
    PROTOTYPES = parse_prototypes(_f.read())
# entry points that return a status and take the launch stream last (call() appends it): name -> argtypes
SIGNATURES = {n: a for n, (r, a, s) in PROTOTYPES.items() if r is ctypes.c_int and s}
# everything else (queries, switches, the profiler): name -> restype
_RESTYPES = {n: r for n, (r, a, s) in PROTOTYPES.items() if n not in SIGNATURES}
EXPORTS = sorted(PROTOTYPES)

_lib = None


def load():
    """Load the shared library (once).  Raises RuntimeError when it is absent or does not match the header."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m ctvae_amd.build` (hipcc, gfx950). "
            "There is no CPU/PyTorch fallback for the ctvae hot path.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise RuntimeError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (restype, argtypes, _) in PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise RuntimeError(f"{LIB_PATH} does not export {name} (stale build?)")
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.ctvae_arch() != b"gfx950":
        raise RuntimeError("libctvae_hip.so was not built for gfx950")
    _lib = lib
    return lib


def check(code: int, what: str):
    if code != 0:
        msg = load().ctvae_error_string(int(code)).decode()
        raise RuntimeError(f"{what} failed: {msg} (code {code})")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


_workspaces = {}


def workspace(device) -> torch.Tensor:
    """Per-(device, stream) scratch buffer.  Kernels on one stream are ordered, so one buffer per stream is
    race-free; a second stream gets its own."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    ws = _workspaces.get(key)
    if ws is None:
        n = load().ctvae_workspace_bytes()
        ws = torch.empty(n // 4, dtype=torch.float32, device=device)
        _workspaces[key] = ws
    return ws


def call(name: str, *args):
    """Launch entry point `name` on the current stream (the trailing stream argument is appended here)."""
    lib = load()
    check(getattr(lib, name)(*args, stream_ptr()), name)


_wino_on = None


def winograd_enable(on: bool) -> bool:
    """Select Winograd (default) or the direct tap-GEMM kernels for the 3x3 stride-1 layers; returns the old setting."""
    global _wino_on
    prev = bool(load().ctvae_winograd_enable(1 if on else 0))
    _wino_on = bool(on)
    return prev


def winograd_enabled() -> bool:
    global _wino_on
    if _wino_on is None:
        lib = load()
        _wino_on = bool(lib.ctvae_winograd_enable(1))
        lib.ctvae_winograd_enable(1 if _wino_on else 0)
    return _wino_on


def prof_enable(on, detailed: bool = False):
    """on=False: off; on=True: per kernel symbol; detailed=True: names also carry the problem shape."""
    load().ctvae_prof_enable((2 if detailed else 1) if on else 0)


def prof_calibrate(n: int = 64):
    """Log n empty event pairs on the current stream (key "(empty event pair)" of the next prof_report())."""
    load().ctvae_prof_calibrate(stream_ptr(), n)


def prof_report() -> dict:
    """{kernel name: dict(count, ms, flops, bytes)} since the last call (synchronises the recorded events)."""
    lib = load()
    buf = ctypes.create_string_buffer(1 << 16)
    lib.ctvae_prof_report(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, cnt, ms, fl, by = line.split("\t")
        out[name] = dict(count=int(cnt), ms=float(ms), flops=float(fl), bytes=float(by))
    return out
