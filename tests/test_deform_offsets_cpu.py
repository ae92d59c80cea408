"""brn_deform_conv2d_offsets_forward (ops.deform_conv2d) without a GPU:
  * the fp64 restatement the GPU tests are judged by (tests/deform_offsets_cases.py) against tests/torch_ref.py::deform_conv2d, against
    F.conv2d at zero offsets (rectangular kernels, per-axis stride / padding, dilation), and G groups fed identical offsets against G = 1;
  * csrc/kernels/deform_sample_geometry.h in a stand-alone program (tests/deform_sample_geometry_main.cpp) built with the host compiler
    under AddressSanitizer / UBSan: against brute force over small maps, on the open ends -1, H, W, and with +-1e30, +-inf, NaN;
  * every refusal of the entry, each checked before the device, and BRN_ERR_NO_DEVICE for a valid call on a host without a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deform_offsets_cases as DC
import torch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "candle_birefnet_amd", "csrc")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(2, 6, 7, 9, 4, 3, 1, 1), (1, 4, 8, 8, 3, 1, 1, 0), (1, 5, 11, 10, 2, 3, 2, 0), (1, 3, 9, 9, 2, 5, 1, 2)],
                         ids=["3x3", "1x1", "stride2", "5x5"])
def test_restatement_equals_torch_ref_on_plain_configurations(cfg):
    B, C, H, W, O, k, s, p = cfg
    c = DC.random_case(1, B, C, 1, k, k, s, p, 1, H, W, O, use_mask=True)
    got = DC.reference(c)
    want = R.deform_conv2d(*(torch.from_numpy(c[n]).double() for n in ("x", "offset", "mask", "weight", "bias")), s, p).numpy()
    assert np.abs(want).max() > 0.1 and np.array_equal(got, want)


@pytest.mark.parametrize("kh,kw,stride,padding,dilation", [(3, 2, (2, 1), (1, 0), (1, 2)), (1, 4, (1, 3), (0, 2), (1, 1)), (3, 3, (1, 1), (2, 2), (2, 2)),
                                                           (2, 5, (3, 2), (2, 1), (3, 1))])
def test_zero_offsets_without_a_mask_are_a_plain_convolution(kh, kw, stride, padding, dilation):
    c = DC.random_case(2, 2, 4, 1, kh, kw, stride, padding, dilation, 10, 11, 3, use_mask=False)
    c["offset"][:] = 0.0
    got = DC.reference(c)
    want = F.conv2d(torch.from_numpy(c["x"]).double(), torch.from_numpy(c["weight"]).double(), torch.from_numpy(c["bias"]).double(), stride=stride,
                    padding=padding, dilation=dilation).numpy()
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("G", [2, 4])
def test_groups_fed_identical_offsets_equal_one_group(G):
    c1 = DC.random_case(3, 2, 8, 1, 3, 2, (2, 1), (1, 0), (1, 2), 9, 7, 5, use_mask=True)
    cg = dict(c1)
    cg["offset"] = np.tile(c1["offset"], (1, G, 1, 1))
    cg["mask"] = np.tile(c1["mask"], (1, G, 1, 1))
    assert np.array_equal(DC.reference(cg), DC.reference(c1))
    # and groups do matter: another offset for the second group moves the result
    cg["offset"][:, c1["offset"].shape[1]:] += 0.5
    assert np.abs(DC.reference(cg) - DC.reference(c1)).max() > 1e-3


# ---- the geometry header ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("deform_geometry") / "deform_sample_geometry")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "deform_sample_geometry_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_geometry_header_against_brute_force_under_sanitizers(report):
    assert report.splitlines()[-1] == "ok"


def test_geometry_every_case_ran(report):
    """20 maps, 9 x 4 x 3 x 4 x 3 output-size cases, 4 x 5 x 6 group layouts"""
    f = report.splitlines()[-2].split()
    assert f[0] == "cases" and int(f[1]) == 20 + 9 * 4 * 3 * 4 * 3 + 4 * 5 * 6 and f[2] == "samples" and int(f[3]) > 20 * 500


# ---- the entry's refusals, all before the device ---------------------------------------------------------------------------------------------
def _call(x=True, offset=True, mask=False, w=True, y=True, B=1, C=4, H=6, W=6, O=2, kh=3, kw=3, stride=(1, 1), pad=(1, 1), dil=(1, 1), G=1, alias=None):
    """brn_deform_conv2d_offsets_forward on small host buffers (the oversized geometries are refused before a byte is read); -> (status, message)"""
    import candle_birefnet_amd as cb
    bx, bo, bm, bw, by = (np.zeros(1 << 16, np.float32) for _ in range(5))      # more than any valid call below touches
    ptr = lambda a, on: a.ctypes.data if on else None
    py = ptr(by, y)
    if alias == "x":
        py = bx.ctypes.data
    elif alias == "offset":
        py = bo.ctypes.data + 4
    elif alias == "mask":
        py = bm.ctypes.data
    st = cb._ffi.lib.brn_deform_conv2d_offsets_forward(ptr(bx, x), B, C, H, W, ptr(bo, offset), ptr(bm, mask), ptr(bw, w), None, O, kh, kw, stride[0], stride[1],
                                                       pad[0], pad[1], dil[0], dil[1], G, py, cb._ffi.BRN_MEM_HOST, 0, None)
    return st, (cb._ffi.lib.brn_last_error() or b"").decode()


BIG = 1 << 16
REFUSALS = [
    (dict(x=False), "null x, offset, w or y"), (dict(offset=False), "null x, offset, w or y"), (dict(w=False), "null x, offset, w or y"),
    (dict(y=False), "null x, offset, w or y"),
    (dict(B=0), "every size >= 1"), (dict(C=0, G=1), "every size >= 1"), (dict(H=0), "every size >= 1"), (dict(W=-3), "every size >= 1"),
    (dict(O=0), "every size >= 1"), (dict(kh=0), "every size >= 1"), (dict(kw=0), "every size >= 1"),
    (dict(stride=(0, 1)), "stride_h, stride_w >= 1"), (dict(stride=(1, -1)), "stride_h, stride_w >= 1"),
    (dict(dil=(0, 1)), "dil_h, dil_w >= 1"), (dict(dil=(1, 0)), "dil_h, dil_w >= 1"),
    (dict(pad=(-1, 0)), "pad_h, pad_w >= 0"), (dict(pad=(0, -1)), "pad_h, pad_w >= 0"),
    (dict(G=0), "offset_groups >= 1"), (dict(G=3), "C % offset_groups == 0"), (dict(G=-2), "offset_groups >= 1"),
    (dict(pad=(0x7fffffff, 1)), "H + 2 pad_h, W + 2 pad_w < 2^31"),
    (dict(kh=9, pad=(1, 1)), "Ho, Wo >= 1"), (dict(kw=4, dil=(1, 3), pad=(0, 0)), "Ho, Wo >= 1"),
    (dict(B=BIG, H=BIG, W=1, C=1, kh=1, kw=1, pad=(0, 0)), "B * Ho * Wo < 2^31"),
    (dict(B=4, C=BIG, G=1, H=128, W=128, kh=1, kw=1, pad=(0, 0)), "B * C * H * W < 2^31"),
    (dict(B=2, C=8, G=8, H=4096, W=4096, kh=3, kw=3), "B * 2 * G * kh * kw * Ho * Wo < 2^31"),
    (dict(O=BIG, C=BIG, kh=1, kw=1, pad=(0, 0), H=2, W=2), "O * C * kh * kw"),
    (dict(O=BIG, B=2, C=1, H=256, W=256, kh=1, kw=1, pad=(0, 0)), "B * O * Ho * Wo < 2^31"),
    (dict(alias="x"), "y must not overlap an input"), (dict(alias="offset"), "y must not overlap an input"),
    (dict(alias="mask", mask=True), "y must not overlap an input"),
]


@pytest.mark.parametrize("kw_,needle", REFUSALS, ids=[f"{i}-{'-'.join(k)}" for i, (k, _) in enumerate(REFUSALS)])
def test_every_refusal_names_its_limit(kw_, needle):
    st, msg = _call(**kw_)
    assert st == 1, (st, msg)                        # BRN_ERR_INVALID_ARG
    assert msg.startswith("deform conv offsets:") and needle in msg, msg


def test_a_valid_call_reaches_the_device():
    """mask and bias may be NULL; without a GPU the answer is BRN_ERR_NO_DEVICE (nothing runs on the CPU), with one the call succeeds"""
    import candle_birefnet_amd as cb
    for kw_ in (dict(), dict(mask=True), dict(G=2, stride=(2, 1), pad=(1, 0), dil=(1, 2), kw=2)):
        st, msg = _call(**kw_)
        if cb.device_count() > 0:
            assert st == 0, msg
        else:
            assert st == 4 and "no CPU fallback" in msg, (st, msg)


def test_ops_signature_is_torchvisions():
    import inspect
    from candle_birefnet_amd import ops
    names = list(inspect.signature(ops.deform_conv2d).parameters)
    assert names[:8] == ["x", "offset", "weight", "bias", "stride", "padding", "dilation", "mask"]
    with pytest.raises(ValueError):
        ops.deform_conv2d(np.zeros((1, 4, 6, 6), np.float32), np.zeros((1, 17, 6, 6), np.float32), np.zeros((2, 4, 3, 3), np.float32), padding=1)
