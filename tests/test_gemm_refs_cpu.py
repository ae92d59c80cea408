"""The GEMM references of kernel_refs.py and the case table of gemm_cases.py, checked without a GPU: every plane-exact case meets its
exactness condition, the reference tells a dropped or an added plane product apart by its bits, the im2col helpers agree with torch, and
kh_pack_weights (tests/gemm_harness/harness.cpp, run as a stand-alone host program under AddressSanitizer / UBSan) lays the weights out as
the plane formats of kernel_refs.py.  Where hipcc is present, the GEMM harness builds."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_cases as GC
import gemm_harness as GH
import kernel_harness as KH
import kernel_refs as KR


def test_case_ids_are_unique_and_the_table_is_small():
    ids = [c.id for c in GC.ALL_CASES]
    assert len(set(ids)) == len(ids)
    assert len(ids) <= 150


@pytest.mark.parametrize("case", GC.ALL_CASES, ids=lambda c: c.id)
def test_exactness_condition_holds(case):
    assert 0 < GC.exactness_margin(case) < 1
    h = GC.host(case, True)
    assert (h["ref"].astype(np.float32).astype(np.float64) == h["ref"]).all() or case.act == KR.ACT_GELU      # the reference itself is an fp32 number


@pytest.mark.parametrize("form", ["bf16x2", "h2"])
def test_chain_is_plane_exact(form):
    h = GC.chain_host(form, True)                     # (asserts both conditions)
    assert np.count_nonzero(h["c1"]) > 0 and (h["ref"].astype(np.float32) == h["ref"]).all()
    assert (np.abs(h["c1"][h["c1"] != 0]) < 1.01).all()


def test_exactness_assert_rejects_dense_rows():
    a = KR.plane_exact_values((8, 96), "bf16x3", 1)
    w = KR.plane_exact_values((8, 96), "bf16x3", 2)
    with pytest.raises(AssertionError):
        KR.assert_plane_exact(a, w, "bf16x3")          # 96 products of magnitude 1 > 64 = 2^24 x 2^-18
    assert KR.assert_plane_exact(a, w, "bf16x2") < 1


def test_plane_exact_values_have_the_planes_they_claim():
    x = KR.plane_exact_values(4096, "bf16x3", 3)
    _, v = KR.split_bf16(x, 3)
    assert set(np.abs(v[0])) == {1.0} and set(np.abs(v[1])) == {0.0, 2.0 ** -9} and set(np.abs(v[2])) == {0.0, 2.0 ** -18}
    assert (v[2][v[1] == 0] == 0).all()
    x = KR.plane_exact_values(4096, "h2", 4)
    _, v = KR.split_h2(x, GC.A_SCALE)
    assert set(np.abs(v[0])) == {GC.A_SCALE} and set(np.abs(v[1])) == {0.0, GC.A_SCALE * 2.0 ** -12}


def _bits(x):
    return np.asarray(x, np.float64).astype(np.float32).view(np.uint32)


@pytest.mark.parametrize("form,dropped,added", [("bf16x3", (1, 1), None), ("bf16x2", (1, 0), (1, 1)), ("h2", (1, 0), None)])
def test_reference_tells_plane_products_apart(form, dropped, added):
    """on plane-exact data, leaving out one kept product (mm of three planes, mh of two, lh of the fp16 pair) or adding a dropped one (mm of two planes)
    changes the fp32 bits of the reference: a kernel that did either cannot pass the bit comparison"""
    case = GC.Case(form, cfg=0)
    h = GC.host(case, True)
    ws = GC.w_scale_of(h["w"])
    av, wv = GC.split_planes(h["a_rows"], form, GC.A_SCALE)[1], GC.split_planes(h["w"], form, ws)[1]
    osc = 1.0 / (GC.A_SCALE * ws) if form == "h2" else 1.0
    full = KR.gemm_planes_ref(av, wv, KR.KEPT[form], osc)
    assert (_bits(full) == _bits(h["ref"])).all()
    less = KR.gemm_planes_ref(av, wv, [k for k in KR.KEPT[form] if k != dropped], osc)
    assert (_bits(less) != _bits(full)).mean() > 0.5
    if added:
        more = KR.gemm_planes_ref(av, wv, list(KR.KEPT[form]) + [added], osc)
        assert (_bits(more) != _bits(full)).mean() > 0.5
    # and on Gaussian data the three-plane mm term stays below the bound the op-level tests use for this mode (3e-5): they cannot see it
    if form == "bf16x3":
        hr = GC.host(case, False)
        av, wv = KR.split_bf16(hr["a_rows"], 3)[1], KR.split_bf16(hr["w"], 3)[1]
        mm = np.abs(KR.gemm_planes_ref(av, wv, [(1, 1)])).max() / max(1.0, np.abs(hr["ref"]).max())
        assert 0 < mm < 3e-5


def test_epilogue_order():
    acc = np.array([[1.0, -2.0], [3.0, 4.0]])
    v = KR.gemm_epilogue_ref(acc, bias=[1, 1], bbias=[[10, 10], [20, 20]], bbias_rows=1, scale=[2, -1], shift=[0.5, 0.5], act=KR.ACT_RELU, R=[[100, 100], [100, 100]])
    assert v.tolist() == [[(1 + 1 + 10) * 2 + 0.5 + 100, 100.0], [(3 + 1 + 20) * 2 + 0.5 + 100, 100.0]]
    g = KR.gemm_epilogue_ref(np.array([[1.0]]), act=KR.ACT_GELU)
    assert abs(g[0, 0] - 0.8413447460685429) < 1e-15


def test_im2col_helpers_match_torch():
    g = np.random.default_rng(0)
    x = g.standard_normal((2, 5, 6, 4))
    w = g.standard_normal((7, 3, 3, 4))                                # [N][ky][kx][ci]
    cols, Ho, Wo = KR.im2col_nhwc(x, 3, 3, 1, 1)
    ref = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(w).permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).reshape(-1, 7).numpy()
    assert (Ho, Wo) == (5, 6) and np.abs(cols @ w.reshape(7, -1).T - ref).max() < 1e-12
    img = g.standard_normal((2, 3, 8, 12))
    wk = g.standard_normal((5, 3, 4, 4))                               # candle's [N][ci][ky][kx]
    cols, Ho, Wo = KR.im2col_nchw(img, 4, 4, 4, 0, 64)
    ref = F.conv2d(torch.from_numpy(img), torch.from_numpy(wk), stride=4).permute(0, 2, 3, 1).reshape(-1, 5).numpy()
    assert (Ho, Wo) == (2, 3) and (cols[:, 48:] == 0).all() and np.abs(cols[:, :48] @ wk.reshape(5, -1).T - ref).max() < 1e-12


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("gemm_pack")
    exe = str(d / "pack_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", KH.CSRC, os.path.join(GH.HDIR, "pack_main.cpp"), "-o", exe])

    def run(w, planes, half):
        src, pad, pl = str(d / "in.f32"), str(d / "pad.f32"), str(d / "planes.u16")
        np.ascontiguousarray(w, np.float32).tofile(src)
        out = subprocess.check_output([exe, src, str(w.shape[0]), str(w.shape[1]), str(planes), str(int(half)), pad, pl])
        npad = (w.shape[0] + 127) // 128 * 128
        return float.fromhex(out.decode().strip()), np.fromfile(pad, np.float32).reshape(npad, -1), np.fromfile(pl, np.uint16).reshape(npad, -1)
    return run


@pytest.mark.parametrize("form", ["f32", "bf16x2", "bf16x3", "h2"])
@pytest.mark.parametrize("exact", [True, False])
def test_pack_weights_decodes_to_the_plane_formats(packer, form, exact):
    N, K = 130, 96
    w = KR.plane_exact_values((N, K), form, 5) if exact else (np.random.default_rng(6).standard_normal((N, K)) * 0.05).astype(np.float32)
    planes, half = GC.FORMS[form]
    s, pad, pl = packer(w, planes, half)
    assert pad.shape == (256, K) and (pad[:N] == w).all() and (pad[N:] == 0).all()
    if not planes:
        assert s == 1.0 and pl.size == 0
        return
    assert s == (GC.w_scale_of(w) if half else 1.0)
    got = KR.decode_planes(pl.view(np.uint8), planes)                                  # a W row is laid out like a P-layout activation row
    want = GC.split_planes(pad, form, s)[0]
    assert got.shape == want.shape == (planes, 256, K) and (got == want).all()


needs_hipcc = pytest.mark.skipif(KH.hipcc() is None, reason="no hipcc")


@needs_hipcc
def test_gemm_harness_builds_beside_the_kernel_harness():
    so = ctypes.CDLL(GH.build())
    assert hasattr(so, "kh_launch_gemm") and hasattr(so, "kh_pack_weights")
    assert os.path.dirname(GH.object_path()) != os.path.dirname(KH.object_path())
    assert os.path.basename(GH.object_path()).startswith("gemm_harness_") and os.path.basename(KH.object_path()).startswith("kernel_harness_")
