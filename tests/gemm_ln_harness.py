"""Loader of the GEMM -> LayerNorm harness: tests/gemm_ln_harness/harness.cpp + kernels/gemm_f32.hip + gemm_split.hip + layernorm.hip, built and found the way kernel_harness.py builds its object.  launch_gemm() is gemm_harness.launch() with one more field,
raw (GemmPlan::raw: the split-K slices stay in ws, no reduce pass); LayerNorm descriptors are given by LayerNormParams' field names."""
import ctypes
import functools
import os

import torch

import gemm_harness as GH
import kernel_harness as KH

HDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_ln_harness")
SOURCES = [os.path.join(HDIR, "harness.cpp")] + [os.path.join(KH.CSRC, "kernels", f) for f in
                                                 ("gemm_f32.hip", "gemm_split.hip", "layernorm.hip")]
GEMM_LN_HARNESS = KH.Harness("gemm_ln_harness", SOURCES)
INVALID_VALUE = 1            # hipErrorInvalidValue

_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


class LayerNorm(ctypes.Structure):
    """KhLayerNorm of the harness = brn::LayerNormParams field by field"""
    _fields_ = [("x", _P), ("y", _P), ("rows", _I), ("C", _I), ("gamma", _P), ("beta", _P), ("eps", _F), ("ldx", _I), ("ldy", _I), ("y_coff", _I),
                ("mode", _I), ("H", _I), ("W", _I), ("Cin", _I), ("y_planes", _I), ("y_h2", _F), ("y_bf16", _I),
                ("part", _P), ("slices", _I), ("bias", _P), ("R", _P), ("ldr", _I), ("r_coff", _I), ("x_out", _P), ("ldxo", _I), ("xo_coff", _I)]


def job(**fields):
    """a descriptor from LayerNormParams' field names; tensors by data_ptr(); eps defaults to 1e-5"""
    fields.setdefault("eps", 1e-5)
    return LayerNorm(**{k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in fields.items()})


def build():
    return GEMM_LN_HARNESS.build()


@functools.lru_cache(maxsize=None)
def lib():
    so, _ = GEMM_LN_HARNESS.load()
    so.kh_launch_gemm_raw.argtypes = [KH._CTYPES[k] for _, k, _ in GH.FIELDS] + [_I]
    so.kh_launch_layernorm_p.argtypes = [ctypes.POINTER(LayerNorm), _P]
    for fn in (so.kh_launch_gemm_raw, so.kh_launch_layernorm_p):
        fn.restype = _I
    return so


def launch_gemm(raw=0, **fields):
    """brn::launch_gemm on the null stream, synchronised; fields as gemm_harness.launch; returns the hipError_t"""
    unknown = set(fields) - {n for n, _, _ in GH.FIELDS}
    assert not unknown, f"not arguments of kh_launch_gemm_raw: {sorted(unknown)}"
    args = []
    for name, _, default in GH.FIELDS:
        v = fields.get(name, default)
        args.append(v.data_ptr() if isinstance(v, torch.Tensor) else v)
    rc = lib().kh_launch_gemm_raw(*args, raw)
    KH.synchronize("launch_gemm")
    return rc


def launch_layernorm(j):
    rc = lib().kh_launch_layernorm_p(ctypes.byref(j), None)
    KH.synchronize("launch_layernorm")
    return rc
