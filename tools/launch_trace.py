"""The recording proxy of the launch-trace probes (tools/train_launch_trace.py, tools/encoder_launch_trace.py): every call
into the HIP library in issue order, with its arguments.  Pointer arguments (device addresses, stream handles) are written
as the ordinal of their first appearance in the trace, NULL as None; integers and floats are written exactly."""
import ctypes

from audiocaption_amd import _lib

trace, ordinals = [], {}


def pointer(v):
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
            trace.append(name + "(" + ", ".join(pointer(v) if k is ctypes.c_void_p else repr(v)
                                                for v, k in zip(a, kinds)) + ")")
            return fn(*a)

        setattr(self, name, call)
        return call
