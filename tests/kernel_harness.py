"""Loader of the test harnesses (class Harness; the GEMM one is set up in gemm_harness.py) and the kernel harness itself: tests/kernel_harness/harness.cpp + kernels/elementwise.hip + kernels/layernorm.hip, compiled from where
they live with the Makefile's own CXXFLAGS into tests/kernel_harness/kernel_harness_<hash>.so, and called through ctypes with raw device
pointers (torch tensors by data_ptr()).  The hash covers the three sources, every header they include and the flags, so a stale object
is never loaded.  With hipcc the object is built on first use; without it an up-to-date object is loaded if there is one; otherwise the
tests that ask for it skip with that reason.  Nothing here touches the product library or its Makefile."""
import ctypes
import functools
import glob
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_build_flags import _flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "candle_birefnet_amd", "csrc")
HDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernel_harness")
SOURCES = [os.path.join(HDIR, "harness.cpp"), os.path.join(CSRC, "kernels", "elementwise.hip"), os.path.join(CSRC, "kernels", "layernorm.hip")]
KERNEL_SOURCES = SOURCES[1:]

# argument kinds: p = device pointer, i = int, f = float, z = size_t, s = the stream (call() fills it in: the null stream)
SIGNATURES = {
    "launch_resize_nhwc": "piiiiiipiiiisii",
    "launch_resize_nchw": "piiipiis",
    "launch_nchw_to_nhwc": "piiiipiisi",
    "launch_nhwc_to_nchw": "piiiiiipsi",
    "launch_image2patches": "piiiiiipiisi",
    "launch_gap_nhwc": "piiiiippsi",
    "launch_small_fc": "piipiiippips",
    "launch_gdt_gate": "piiiipipfsi",
    "launch_pixel_dot": "piiiipfpsi",
    "launch_final_head": "piiipfiiips",
    "launch_head_stencil5x5": "piiippps",
    "launch_f32_to_bf16": "pzpsi",
    "launch_bf16_to_f32": "pzpsi",
    "launch_sigmoid": "pzps",
    "launch_mod_sigmoid2": "pziiis",
    "launch_layernorm": "ppiippfiiiiiiiifis",
}
_CTYPES = {"p": ctypes.c_void_p, "s": ctypes.c_void_p, "i": ctypes.c_int, "f": ctypes.c_float, "z": ctypes.c_ulonglong}


def hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def build_flags():
    return [*_flags(), "-fPIC", "-I", CSRC]


def _with_headers(paths):
    """the files and, recursively, every quoted #include that resolves next to the includer or under csrc/"""
    seen, todo = [], list(paths)
    while todo:
        f = os.path.normpath(todo.pop())
        if f in seen:
            continue
        seen.append(f)
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(f).read(), re.M):
            for base in (os.path.dirname(f), CSRC):
                cand = os.path.join(base, inc)
                if os.path.exists(cand):
                    todo.append(cand)
                    break
    return sorted(seen)


class Harness:
    """One shared object tests/<name>/<name>_<hash>.so: `sources` (the first is the harness file under tests/<name>/, the others are kernel
    files taken from where they live) compiled together with the Makefile's own flags"""

    def __init__(self, name, sources):
        self.name, self.sources, self.hdir = name, list(sources), os.path.dirname(sources[0])

    def object_path(self):
        h = hashlib.sha256(" ".join(build_flags()[:-1]).encode())      # (not the -I path: it differs between checkouts)
        for f in _with_headers(self.sources):
            h.update(os.path.relpath(f, ROOT).encode() + b"\0" + open(f, "rb").read() + b"\0")
        return os.path.join(self.hdir, f"{self.name}_{h.hexdigest()[:16]}.so")

    def build(self):
        """compile the object if it is not there yet; returns its path (needs hipcc)"""
        out = self.object_path()
        if not os.path.exists(out):
            tmp = os.path.join(self.hdir, f"tmp{os.getpid()}_{self.name}.so")       # (git-ignored like the object itself)
            subprocess.run([hipcc(), *build_flags(), "-x", "hip", "-shared", *self.sources, "-o", tmp, "-Wl,-rpath,/opt/rocm/lib"],
                           check=True, capture_output=True, timeout=900)
            os.replace(tmp, out)
            for old in glob.glob(os.path.join(self.hdir, f"{self.name}_*.so")):
                if old != out:
                    os.remove(old)
        return out

    def load(self):
        """(the ctypes library, "built" or "loaded"); skips the calling test when the object can be neither built nor found"""
        out = self.object_path()
        route = "loaded" if os.path.exists(out) else "built"
        if not os.path.exists(out):
            if hipcc() is None:
                pytest.skip(f"{self.name.replace('_', ' ')}: no hipcc and no up-to-date {os.path.basename(out)}")
            self.build()
        return ctypes.CDLL(out), route


KERNEL_HARNESS = Harness("kernel_harness", SOURCES)


def object_path():
    return KERNEL_HARNESS.object_path()


def build():
    return KERNEL_HARNESS.build()


ROUTE = None     # "built" or "loaded", once lib() has run


@functools.lru_cache(maxsize=None)
def lib():
    """the loaded harness; skips the calling test when it can be neither built nor found"""
    global ROUTE
    so, ROUTE = KERNEL_HARNESS.load()
    for name, sig in SIGNATURES.items():
        fn = getattr(so, "kh_" + name)
        fn.argtypes = [_CTYPES[c] for c in sig]
        fn.restype = ctypes.c_int
    so.kh_gap_scratch_floats.argtypes = [ctypes.c_int] * 3
    so.kh_gap_scratch_floats.restype = ctypes.c_ulonglong
    return so


def launcher_names():
    """every launch_* that the two kernel files define (hipError_t launch_x(...) {)"""
    names = []
    for f in KERNEL_SOURCES:
        names += re.findall(r"^\s*hipError_t\s+(launch_\w+)\s*\(", open(f).read(), re.M)
    return sorted(set(names))


def synchronize(name):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a device fault: nothing more may run on this GPU from this process
        pytest.exit(f"{name}: {e}", returncode=3)


def call(name, *args):
    """run one launcher on the null stream and synchronise; args are the wrapper's without the stream; returns the hipError_t"""
    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    conv.insert(SIGNATURES[name].index("s"), None)
    assert len(conv) == len(SIGNATURES[name]), f"{name}: {len(conv)} arguments for {SIGNATURES[name]}"
    rc = getattr(lib(), "kh_" + name)(*conv)
    synchronize(name)
    return rc


def run(name, *args):
    rc = call(name, *args)
    assert rc == 0, f"{name} returned hipError_t {rc}"


# ---- device buffers with a sentinel bit pattern (a NaN in all three types) in and around them ----
FORMS = [("f32", 0, torch.float32), ("bf16", 1, torch.bfloat16), ("f16", 2, torch.float16)]
SENT32, SENT16 = np.array(0xFFC5A5A5, np.uint32).view(np.int32)[()], np.array(0xFFA5, np.uint16).view(np.int16)[()]
GUARD = 64       # elements before and after every guarded buffer


def _ity(dt):
    return torch.int32 if dt == torch.float32 else torch.int16


def sentinel(dt):
    return SENT32 if dt == torch.float32 else SENT16


class Guarded:
    """`t`: a sentinel-filled device tensor of `shape` with GUARD sentinel elements on both sides"""

    def __init__(self, shape, dt):
        n = int(np.prod(shape))
        self.dt = dt
        self.full = torch.full((n + 2 * GUARD,), int(sentinel(dt)), dtype=_ity(dt), device="cuda").view(dt)
        self.t = self.full[GUARD:GUARD + n].view(*shape)

    def bits(self):
        return self.t.view(_ity(self.dt)).cpu().numpy()

    def assert_guards(self):
        b = self.full.view(_ity(self.dt)).cpu().numpy()
        assert (b[:GUARD] == sentinel(self.dt)).all() and (b[-GUARD:] == sentinel(self.dt)).all(), "wrote outside the buffer"

    def assert_untouched_outside(self, window):
        """every element outside t[window] (an index expression) and both guard zones still hold the sentinel bits"""
        self.assert_guards()
        b = self.bits().copy()
        if window is not None:
            b[window] = sentinel(self.dt)
        bad = np.argwhere(b != sentinel(self.dt))
        assert bad.size == 0, f"{len(bad)} elements outside the window were written, first at {bad[0].tolist()}"


def bits_of(t):
    return t.contiguous().view(_ity(t.dtype)).cpu().numpy()


def dev(a, dt=torch.float32):
    """host array -> device tensor of storage type dt (RNE)"""
    return torch.as_tensor(np.asarray(a)).to(dt).cuda()


def rnd(*shape, seed=0, std=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * std).astype(np.float32)


def windowed(vals, ld, coff, dt, seed=99):
    """vals [..., C] -> a device tensor [..., ld] of type dt whose columns [coff, coff+C) hold vals (RNE) and whose other columns hold
    large finite noise (a read outside the window shows); returns (tensor, the window's exact values as float64)"""
    vals = np.asarray(vals, np.float32)
    C = vals.shape[-1]
    host = rnd(*vals.shape[:-1], ld, seed=seed, std=1e3)
    host[..., coff:coff + C] = vals
    t = dev(host, dt)
    return t, t[..., coff:coff + C].double().cpu().numpy()


def report(kernel, form, err):
    print(f"KH_MAXERR {kernel} {form} {float(err):.3e}")
