"""The recording proxy of the launch-trace probes (tools/train_launch_trace.py, tools/encoder_launch_trace.py,
tools/decode_launch_trace.py): every call into the HIP library in issue order, with its arguments.  Pointer arguments
(device addresses, stream handles) are written as the ordinal of their first appearance in the trace, NULL as None; integers
and floats are written exactly.  A struct passed by reference is written as its type and a digest of its fields (addresses
as ordinals again), a table of addresses as the list of its entries."""
import ctypes
import hashlib

from audiocaption_amd import _lib

trace, ordinals = [], {}
_SCALARS = (ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_ulonglong)


def _fields(s):
    for name, kind in s._fields_:
        v = getattr(s, name)
        if isinstance(v, ctypes.Array):
            for e in v:
                yield from _fields(e)
        else:
            yield pointer(v) if kind is ctypes.c_void_p else repr(v)


def pointer(v):
    if isinstance(v, ctypes.Array):
        return "[" + ", ".join(pointer(e) for e in v) + "]"
    if hasattr(v, "_obj"):               # ctypes.byref(struct)
        return type(v._obj).__name__ + ":" + hashlib.sha256(",".join(_fields(v._obj)).encode()).hexdigest()[:12]
    v = v.value if isinstance(v, ctypes.c_void_p) else v
    if not v:
        return "None"
    return f"p{ordinals.setdefault(int(v), len(ordinals))}"


class TracingLib:
    """Forwards every call to the real library and records (symbol, normalised arguments)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        kinds = _lib.SIGNATURES[name][1]

        def call(*a):
            assert len(a) == len(kinds), name
            trace.append(name + "(" + ", ".join(repr(v) if k in _SCALARS else pointer(v)
                                                for v, k in zip(a, kinds)) + ")")
            return fn(*a)

        setattr(self, name, call)
        return call
