"""ctypes binding of libhmmc_hip.so — the C-ABI declared in include/hmmc_hip.h.

The product path has no CPU fallback: if the library is missing, `load()` raises.
PyTorch only supplies device memory (tensor.data_ptr()) and the current HIP stream.
"""
from __future__ import annotations

import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HMMC_LIB") or os.path.join(_HERE, "libhmmc_hip.so")     # HMMC_LIB: a variant build (A/B runs, scratch/)

_C = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_long, "f": ctypes.c_float, "z": ctypes.c_size_t, "s": ctypes.c_char_p}

HEADER = os.path.join(_HERE, "..", "include", "hmmc_hip.h")
_CODE = {"int": "i", "long": "l", "float": "f", "size_t": "z"}


def _parse_header(path=HEADER):
    """include/hmmc_hip.h -> (SIGNATURES: name -> (argument codes, return code) of every entry point, ERRORS: HMMC_ERR_* value ->
    the message in its comment, EPI: "EPI_<flag>" -> the value of HMMC_EPI_<flag>, STATUS: "HMMC_ERR_<name>" -> its value).
    Argument codes are keys of _C: "p" any pointer (hmmc_stream_t included), "s" const char*."""
    src = open(path).read()
    defs = re.findall(r"#define (HMMC_ERR_\w+) \((-\d+)\)\s*/\*\s*(.*?)\s*\*/", src)
    errors = {int(v): msg for _, v, msg in defs}
    status = {name: int(v) for name, v, _ in defs}
    epi = {"EPI_" + name: int(v) for name, v in re.findall(r"#define HMMC_EPI_(\w+) (\d+)", src)}
    sigs = {}
    for ret, name, args in re.findall(r"\b(int|size_t)\s+(hmmc_\w+)\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", src, flags=re.S)):
        codes = ""
        for a in [x.strip() for x in args.split(",") if x.strip() not in ("", "void")]:
            if a.startswith("const char*"):
                codes += "s"
            elif "*" in a or "hmmc_stream_t" in a:
                codes += "p"
            else:
                codes += _CODE[a.split()[-2] if len(a.split()) > 1 else a]
        sigs[name] = (codes, _CODE[ret])
    return sigs, errors, epi, status


SIGNATURES, ERRORS, EPI, STATUS = _parse_header()
TOPN_MAX = int(re.search(r"#define HMMC_TOPN_MAX (\d+)", open(HEADER).read()).group(1))      # longest list of hmmc_topn_select

# The library reads no environment variable itself (include/hmmc_hip.h: hmmc_set_option).  These A/B switches of scratch/ runs
# and tests are translated once, when the library is loaded; a variable that is PRESENT (any value, the empty string included)
# switches its option on - the same rule hmmc_amd/functional.py applies on its side.
ENV_OPTIONS = {"HMMC_NO_WGRAD_GROUP": "no_wgrad_group", "HMMC_NO_F32_WAVEK": "no_f32_wavek", "HMMC_NO_F32_DMA": "no_f32_dma",
               "HMMC_NO_LEAD_ATTN": "no_lead_attn"}


def set_option(key, value):
    """hmmc_set_option(key, value): process-wide A/B switch of the library (see ENV_OPTIONS for the keys)."""
    rc = load().hmmc_set_option(key.encode(), int(bool(value)))
    if rc != 0:
        raise KeyError(f"hmmc_set_option: unknown option {key!r}")


def get_option(key):
    rc = load().hmmc_get_option(key.encode())
    if rc < 0:
        raise KeyError(f"hmmc_get_option: unknown option {key!r}")
    return bool(rc)

_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m hmmc_amd.build` (hipcc, gfx950). "
                "hmmc_amd has no CPU or eager fallback.")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (args, ret) in SIGNATURES.items():
            fn = getattr(lib, name)            # AttributeError here = header/library mismatch
            fn.argtypes = [_C[c] for c in args]
            fn.restype = _C[ret]
        _lib = lib
        for var, key in ENV_OPTIONS.items():
            if var in os.environ:
                lib.hmmc_set_option(key.encode(), 1)
    return _lib


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call_status(name, *args, allow=None):
    """Call an int-returning entry point on the current stream -> its status: 0, or the HMMC_ERR_* named `allow` (the caller has
    another way); raise on any other."""
    rc = getattr(load(), name)(*args, stream())
    if rc != 0 and (allow is None or rc != STATUS[allow]):
        raise RuntimeError(f"{name} failed: {ERRORS.get(rc, rc)}")
    return rc


def call(name, *args):
    """Call an int-returning entry point on the current stream; raise on a non-zero status."""
    rc = getattr(load(), name)(*args, stream())
    if rc != 0:
        raise RuntimeError(f"{name} failed: {ERRORS.get(rc, rc)}")


def query(name, *args):
    return getattr(load(), name)(*args)
