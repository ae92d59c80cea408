"""Loader of the 16-bit GEMM harness: tests/gemm_s16_harness/harness.cpp + kernels/gemm_bf16.hip as is (namespace brn, bf16) + gemm_f16.cpp,
which compiles the same kernel file with BRN_S16_F16=1 (namespace brn::hf, fp16) — built and found the way kernel_harness.py builds its object
(class Harness: one hash over sources, headers and flags; skip when it can neither be built nor found).  launch() calls launch_gemm_bf16 of
either build with every GemmParams field the 16-bit kernels read, the plan given by name and the CU count of the persistent grid; pack() lays a
host weight matrix out with the product's own pack_s16_storage (brn_pack.h); plan() is the product's tile planner."""
import ctypes
import functools
import os

import numpy as np
import torch

import kernel_harness as KH

HDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_s16_harness")
SOURCES = [os.path.join(HDIR, "harness.cpp"), os.path.join(KH.CSRC, "kernels", "gemm_bf16.hip"), os.path.join(HDIR, "gemm_f16.cpp")]
GEMM_S16_HARNESS = KH.Harness("gemm_s16_harness", SOURCES)

DENSE, CONV_NHWC, GATHER_NCHW = 0, 1, 2
INVALID_VALUE = 1            # hipErrorInvalidValue
TILES = {0: (128, 128), 1: (128, 64), 2: (256, 256), 3: (256, 192)}          # cfg -> (BM, BN)
WG_PER_CU = {0: 2, 1: 3, 2: 1, 3: 1}                                          # persistent workgroups per CU (launch_bf16_cfg: LDS-limited)

# kh_launch_gemm_s16's arguments in order: (name, kind, default); kinds as in kernel_harness.SIGNATURES
FIELDS = [
    ("f16", "i", 0), ("A", "p", None), ("Wp", "p", None), ("C", "p", None), ("M", "i", 0), ("N", "i", 0), ("K", "i", 0), ("mode", "i", DENSE),
    ("lda", "i", 0), ("a_coff", "i", 0),
    ("Hin", "i", 0), ("Win", "i", 0), ("Cin", "i", 0), ("kh", "i", 0), ("kw", "i", 0), ("stride", "i", 1), ("pad", "i", 0), ("dil", "i", 1),
    ("Hout", "i", 0), ("Wout", "i", 0),
    ("bias", "p", None), ("bbias", "p", None), ("bbias_rows", "i", 1), ("scale", "p", None), ("shift", "p", None), ("act", "i", 0),
    ("R", "p", None), ("ldr", "i", 0), ("r_coff", "i", 0), ("ldc", "i", 0), ("c_coff", "i", 0),
    ("wp_rows", "i", 0), ("wp_ld", "i", 0), ("k_chunk_major", "i", 0), ("c_f32", "i", 0), ("r_f32", "i", 0),
    ("cfg", "i", 0), ("splitk", "i", 1), ("ws", "p", None), ("launch_cus", "i", 256), ("stream", "s", None),
]


def object_path():
    return GEMM_S16_HARNESS.object_path()


def build():
    return GEMM_S16_HARNESS.build()


def _declare(so):
    so.kh_launch_gemm_s16.argtypes = [KH._CTYPES[k] for _, k, _ in FIELDS]
    so.kh_launch_gemm_s16.restype = ctypes.c_int
    ip = ctypes.POINTER(ctypes.c_int)
    so.kh_pack_s16.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ip, ip, ip]
    so.kh_pack_s16.restype = ctypes.c_int
    so.kh_plan_gemm_s16.argtypes = [ctypes.c_int] * 5 + [ip, ip]
    so.kh_plan_gemm_s16.restype = None
    return so


@functools.lru_cache(maxsize=None)
def lib():
    so, _ = GEMM_S16_HARNESS.load()
    return _declare(so)


def launch(**fields):
    """launch_gemm_bf16 (f16 = 0: brn, 1: brn::hf) on the null stream, synchronised; fields by GemmParams' names (+ cfg, splitk, ws, launch_cus),
    tensors by data_ptr(); returns the hipError_t"""
    unknown = set(fields) - {n for n, _, _ in FIELDS}
    assert not unknown, f"not arguments of kh_launch_gemm_s16: {sorted(unknown)}"
    args = []
    for name, _, default in FIELDS:
        v = fields.get(name, default)
        args.append(v.data_ptr() if isinstance(v, torch.Tensor) else v)
    rc = lib().kh_launch_gemm_s16(*args)
    KH.synchronize("launch_gemm_bf16")
    return rc


def pack_host(w, f16, conv_taps=0, cinp=0):
    """host fp32 [N][K] (conv: K order (tap, channel)) -> (uint16 [rows][ld] as pack_s16_storage lays it out, chunk_major)"""
    w = np.ascontiguousarray(w, np.float32)
    N, K = w.shape
    rows, ld, cm = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib().kh_pack_s16(w.ctypes.data, N, K, int(f16), conv_taps, cinp, None, rows, ld, cm) == 0
    out = np.empty((rows.value, ld.value), np.uint16)
    assert lib().kh_pack_s16(w.ctypes.data, N, K, int(f16), conv_taps, cinp, out.ctypes.data, rows, ld, cm) == 0
    return out, bool(cm.value)


def pack(w, f16, conv_taps=0, cinp=0):
    """-> dict(Wp = the device matrix (int16 words), wp_rows, wp_ld, k_chunk_major): the launch fields of the weights"""
    out, cm = pack_host(w, f16, conv_taps, cinp)
    return dict(Wp=torch.from_numpy(out.view(np.int16)).cuda(), wp_rows=out.shape[0], wp_ld=out.shape[1], k_chunk_major=int(cm))


def plan(M, N, K, f32_residual=False, gelu=False):
    """plan_gemm_bf16 -> (cfg, splitk)"""
    cfg, sk = ctypes.c_int(), ctypes.c_int()
    lib().kh_plan_gemm_s16(M, N, K, int(f32_residual), int(gelu), cfg, sk)
    return cfg.value, sk.value
