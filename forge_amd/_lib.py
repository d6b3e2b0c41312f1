"""ctypes binding of libforge_hip.so (include/forge_hip.h). No fallbacks: if the library is
missing or a call fails, a RuntimeError is raised — the product never routes through a CPU path."""
import ctypes
import os
import re

# torch FIRST: PyTorch-ROCm ships its own libamdhip64; libforge_hip.so must bind to the HIP runtime that
# owns torch's streams and allocations. Loading our library before torch would pull in /opt/rocm's copy
# and every launch on a torch stream would fail with "no ROCm-capable device is detected".
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FORGE_AMD_LIB") or os.path.join(_HERE, "libforge_hip.so")     # override: instrumented debug builds (tools/debug)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "forge_hip.h")
_lib = None

_PARAMS = {"forge_stream_t": ctypes.c_void_p, "long long": ctypes.c_longlong, "int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double}
_RESULTS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "const char*": ctypes.c_char_p}
_PARAM = re.compile(r"(%s)(?: (?!(?:unsigned|signed|short|long|int|char|float|double)\b)\w+)?" % "|".join(_PARAMS))     # a scalar type, then a name that is no type word
_DECLARATION = re.compile(r"(.*?) ?\b(forge_\w+) ?\(([^()]*)\)")                        # <result> forge_<name>(<params>): no nested parentheses


def parse_header(text):
    """{name: (restype, argtypes)} of every `<result> forge_<name>(<params>);` of the header text. This reads the header's own subset of C (its
    conventions promise plain C types), not C: what is outside the subset raises - it is never skipped and never guessed, because a wrong class
    here hands a kernel a garbage stride or byte count."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)                  # preprocessor lines, continued ones included
    text = re.sub(r'extern\s+"C"\s*\{|\}', " ", text)
    out = {}
    for decl in (" ".join(d.split()) for d in text.split(";")):
        if not decl or decl == "typedef void* forge_stream_t":
            continue
        m = _DECLARATION.fullmatch(decl)
        result = m and m.group(1).replace(" *", "*")
        params = [] if not m or m.group(3).strip() in ("", "void") else [p.strip() for p in m.group(3).split(",")]
        if not m or result not in _RESULTS or not all("*" in p or _PARAM.fullmatch(p) for p in params):
            raise RuntimeError("forge_amd: `%s;` in the header is not `<result> forge_<name>(<params>)` over the plain C types the ctypes binding "
                               "is derived from (parameters: pointers, forge_stream_t, int, long long, float, double; results: int, long long, "
                               "const char*). A new type is a decision to make in forge_amd/_lib.py." % decl)
        out[m.group(2)] = (_RESULTS[result], [ctypes.c_void_p if "*" in p else _PARAMS[_PARAM.fullmatch(p).group(1)] for p in params])
    return out


def load_header(path):
    """parse_header of the file at path."""
    if not os.path.exists(path):
        raise RuntimeError("forge_amd: %s not found. The ctypes binding of libforge_hip.so is derived from this header's declarations; "
                           "the package runs from its source tree." % path)
    with open(path) as f:
        return parse_header(f.read())


# The one reading of include/forge_hip.h, once per process. Adding an entry point means declaring it there (and defining it in csrc/): nothing here.
PROTOTYPES = load_header(HEADER_PATH)                                                 # name -> (restype, argtypes)
SIGNATURES = {name: args for name, (_, args) in PROTOTYPES.items()}                   # name -> argtypes
_LL_RESULTS = tuple(name for name, (res, _) in PROTOTYPES.items() if res is ctypes.c_longlong)     # byte and element counts


def lib():
    """Load (once) and return the ctypes handle. Raises if the library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "forge_amd: %s not found. Build it with `python -m forge_amd.build` (needs hipcc, "
                "targets gfx950). There is no CPU/PyTorch fallback for the HIP kernels." % LIB_PATH)
        h = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(h, name)
            fn.argtypes, fn.restype = args, res
        _lib = h
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().forge_last_error().decode("utf-8", "replace")
        raise RuntimeError("forge_amd: %s failed (code %d): %s" % (what, rc, msg))


def size_query(name, *args):
    """A host-side size query of the library: a negative result is an error code, raised with the library's message."""
    b = int(getattr(lib(), name)(*args))
    if b < 0:
        check(b, name)
    return b


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def current_stream():
    """torch's current stream of the CURRENT device (launchers run under on_tensor_device, which makes the operands' device current)."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def on_tensor_device(fn):
    """Decorator for launch wrappers: run `fn` with the device of its first cuda tensor argument (positional or keyword) current, so that
    `current_stream()` is that device's stream and per-device kernel attributes are applied to it (a process may hold models on
    several GPUs while torch's current device is another one)."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kw):
        for a in list(args) + list(kw.values()):       # keyword call sites too (the models call rotate / render with keywords)
            if torch.is_tensor(a) and a.is_cuda:
                if a.device.index != torch.cuda.current_device():
                    with torch.cuda.device(a.device):
                        return fn(*args, **kw)
                break
        return fn(*args, **kw)
    return wrapped
