"""ctypes binding of libdecagon_hip.so (include/decagon_hip.h and its extension headers,
include/decagon_hip_ext.h and include/decagon_hip_ext2.h).

This is the one place the Python layer touches native code.  There is no fallback: if the
library is missing or fails to load, importing the compute path raises, and every op of the
package fails loudly instead of silently running on the CPU.
"""
from __future__ import annotations

import ctypes
import threading
from pathlib import Path

from . import _build, abi
# name -> (restype, argtypes), as include/decagon_hip.h and the extension headers declare them
SIGNATURES = {name: (p.restype, p.argtypes) for name, p in abi.ALL_PROTOTYPES.items()}
from .tuning import knob

ABI_VERSION = 39  # what this Python layer expects of dg_abi_version()
globals().update(abi.CONSTANTS)  # every DG_* macro of the header
globals().update(abi.STRUCTS)    # DgRelGroup, ...: the ctypes.Structure of every dg_* struct
for _ext in abi.EXTENSIONS:  # decagon_hip_ext.h, decagon_hip_ext2.h
    globals().update(_ext.constants)
    globals().update({cls.__name__: cls for cls in _ext.structs.values()})

_ERRS = {code: name for name, code in abi.CONSTANTS.items() if name.startswith("DG_E") and code < 0}


def arg_index(name: str, param: str) -> int:
    """The position of parameter `param` of entry point `name`."""
    if param not in abi.ALL_PROTOTYPES[name].names:
        raise TypeError(f"{name} has no parameter {param!r}")
    return abi.ALL_PROTOTYPES[name].names.index(param)


def pack(name: str, **values) -> list:
    """The positional argument list of entry point `name` from its arguments by parameter name."""
    names = abi.ALL_PROTOTYPES[name].names
    missing, unknown = [p for p in names if p not in values], [v for v in values if v not in names]
    if missing or unknown:
        raise TypeError(f"{name}: missing arguments {missing}, unknown arguments {unknown}")
    return [values[p] for p in names]


_LIB = None
_LOAD_LOCK = threading.Lock()  # staged_layout's thread pool may make the first call


class KernelError(RuntimeError):
    pass


def load(build_if_missing: bool = True) -> ctypes.CDLL:
    """Load (building first if needed and allowed) and type the native library."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LOAD_LOCK:
        if _LIB is None:
            _LIB = _load(build_if_missing)
    return _LIB


def _load(build_if_missing: bool) -> ctypes.CDLL:
    override = knob("DG_LIB", "")  # an instrumented build (scripts/staged_prof.py)
    path = Path(override) if override else _build.lib_path()
    if not override and (not path.exists() or (build_if_missing and _build.needs_build())):
        if not build_if_missing:
            raise ImportError(f"{path} missing: run __graft_entry__.build() or python -m decagon_amd._build")
        _build.build()
    lib = ctypes.CDLL(str(path))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    got = lib.dg_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"libdecagon_hip ABI {got} != expected {ABI_VERSION}; rebuild")
    return lib


def check(rc: int, what: str) -> None:
    if rc != DG_OK:
        name = _ERRS.get(rc, f"hipError_t {rc}")
        raise KernelError(f"{what} failed: {name}")
