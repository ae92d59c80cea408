"""Loader of the GEMM harness: tests/gemm_harness/harness.cpp + kernels/gemm_f32.hip + kernels/gemm_split.hip, built and found the way
kernel_harness.py builds its object (class Harness: one hash over sources, headers and flags; skip when it can neither be built nor found).
launch() calls brn::launch_gemm with every GemmParams field and the plan given by name; pack_weights() lays a host weight matrix out with the
product's own packers (brn_pack.h) and uploads it."""
import ctypes
import functools
import os

import numpy as np
import torch

import kernel_harness as KH

HDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_harness")
SOURCES = [os.path.join(HDIR, "harness.cpp"), os.path.join(KH.CSRC, "kernels", "gemm_f32.hip"), os.path.join(KH.CSRC, "kernels", "gemm_split.hip")]
GEMM_HARNESS = KH.Harness("gemm_harness", SOURCES)

DENSE, CONV_NHWC, GATHER_NCHW = 0, 1, 2
INVALID_VALUE = 1            # hipErrorInvalidValue

# kh_launch_gemm's arguments in order: (name, kind, default); kinds as in kernel_harness.SIGNATURES
FIELDS = [
    ("A", "p", None), ("W", "p", None), ("C", "p", None), ("M", "i", 0), ("N", "i", 0), ("K", "i", 0), ("mode", "i", DENSE), ("lda", "i", 0), ("a_coff", "i", 0),
    ("Hin", "i", 0), ("Win", "i", 0), ("Cin", "i", 0), ("kh", "i", 0), ("kw", "i", 0), ("stride", "i", 1), ("pad", "i", 0), ("dil", "i", 1),
    ("Hout", "i", 0), ("Wout", "i", 0), ("Kreal", "i", 0),
    ("bias", "p", None), ("bbias", "p", None), ("bbias_rows", "i", 0), ("scale", "p", None), ("shift", "p", None), ("act", "i", 0),
    ("R", "p", None), ("ldr", "i", 0), ("r_coff", "i", 0), ("ldc", "i", 0), ("c_coff", "i", 0),
    ("Wp", "p", None), ("planes", "i", 0), ("wp_rows", "i", 0), ("a_planes", "i", 0), ("c_planes", "i", 0),
    ("h2", "i", 0), ("a_scale", "f", 0.0), ("out_scale", "f", 0.0), ("c_bf16", "i", 0),
    ("cfg", "i", 2), ("splitk", "i", 1), ("ws", "p", None), ("stream", "s", None),
]


def object_path():
    return GEMM_HARNESS.object_path()


def build():
    return GEMM_HARNESS.build()


@functools.lru_cache(maxsize=None)
def lib():
    so, _ = GEMM_HARNESS.load()
    so.kh_launch_gemm.argtypes = [KH._CTYPES[k] for _, k, _ in FIELDS]
    so.kh_launch_gemm.restype = ctypes.c_int
    so.kh_pack_weights.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    so.kh_pack_weights.restype = ctypes.c_float
    return so


def launch(**fields):
    """brn::launch_gemm on the null stream, synchronised; fields by GemmParams' names (+ cfg, splitk, ws), tensors by data_ptr(); returns the hipError_t"""
    unknown = set(fields) - {n for n, _, _ in FIELDS}
    assert not unknown, f"not arguments of kh_launch_gemm: {sorted(unknown)}"
    args = []
    for name, _, default in FIELDS:
        v = fields.get(name, default)
        args.append(v.data_ptr() if isinstance(v, torch.Tensor) else v)
    rc = lib().kh_launch_gemm(*args)
    KH.synchronize("launch_gemm")
    return rc


def pack_weights(w, planes=0, half=False):
    """host fp32 [N][K] -> dict(W = the fp32 matrix padded to 128 rows, Wp = its planes (int16 words) or None, wp_rows, w_scale), on the device"""
    w = np.ascontiguousarray(w, np.float32)
    N, K = w.shape
    npad = (N + 127) // 128 * 128
    w_pad = np.empty((npad, K), np.float32)
    pl = np.empty((npad, K * planes), np.uint16) if planes else None
    s = lib().kh_pack_weights(w.ctypes.data, N, K, planes, int(half), w_pad.ctypes.data, pl.ctypes.data if planes else None)
    assert s > 0, "kh_pack_weights refused its arguments"
    return dict(W=torch.from_numpy(w_pad).cuda(), Wp=torch.from_numpy(pl.view(np.int16)).cuda() if planes else None, wp_rows=npad, w_scale=float(s),
                host_pad=w_pad, host_planes=pl)
