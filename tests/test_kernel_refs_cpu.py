"""The references and format emulations of kernel_refs.py, checked without a GPU; and, where hipcc is present, that the kernel harness builds
and wraps every launcher of kernels/elementwise.hip and kernels/layernorm.hip."""
import ctypes

import numpy as np
import pytest
import torch

import kernel_harness as KH
import kernel_refs as KR
import torch_ref as R


def _normal_range(n, seed):
    g = np.random.default_rng(seed)
    return (g.standard_normal(n) * np.exp2(g.integers(-20, 20, n))).astype(np.float32)


@pytest.mark.parametrize("NP", [2, 3])
def test_plane_decoder_inverts_the_encoder(NP):
    planes = np.random.default_rng(NP).integers(0, 65536, (NP, 3, 96)).astype(np.uint16)
    raw = KR.encode_planes(planes)
    assert raw.shape == (3, 96 * 2 * NP)
    assert (KR.decode_planes(raw, NP) == planes).all()
    # one element by hand: plane 1, column 37 = tile 1, element 5
    assert raw[2, 64 * NP + 64 + 10] | (raw[2, 64 * NP + 64 + 11].astype(np.uint16) << 8) == planes[1, 2, 37]


def test_three_bf16_planes_are_exact():
    x = _normal_range(100000, 1)
    bits, vals = KR.split_bf16(x, 3)
    assert (vals.astype(np.float64).sum(0) == x.astype(np.float64)).all()
    assert (KR.bf16_bits_to_f64(bits) == vals).all()


def test_two_bf16_planes_within_2pow17():
    x = _normal_range(100000, 2)
    _, vals = KR.split_bf16(x, 2)
    err = np.abs(vals.astype(np.float64).sum(0) - x.astype(np.float64))
    assert (err <= 2.0 ** -17 * np.abs(x.astype(np.float64))).all()     # two RNE roundings, each leaves at most 2^-9 of what it rounds
    assert (vals[0] == torch.from_numpy(x).to(torch.bfloat16).float().numpy()).all()


@pytest.mark.parametrize("s", [8.0, 0.5])
def test_h2_pair_within_2pow21(s):
    g = np.random.default_rng(3)
    x = (g.standard_normal(100000) * 4).astype(np.float32)
    bits, vals = KR.split_h2(x, s)
    sx = x.astype(np.float64) * s
    big = np.abs(sx) >= 2.0 ** -3
    err = np.abs(vals.astype(np.float64).sum(0) - sx)
    assert big.sum() > 50000 and (err[big] <= 2.0 ** -21 * np.abs(sx[big])).all()
    assert (err[~big] <= 2.0 ** -25).all()
    assert (KR.f16_bits_to_f64(bits) == vals).all()


@pytest.mark.parametrize("Cimg,H,W,th,tw,cpad", [(3, 4, 144, 2, 72, 16), (3, 32, 32, 4, 4, 192), (3, 48, 48, 8, 8, 128)])
def test_image2patches_matches_torch_ref(Cimg, H, W, th, tw, cpad):
    x = np.random.default_rng(4).standard_normal((2, Cimg, H, W))
    y = KR.image2patches_nhwc(x, th, tw, cpad)
    ref = R.image2patches(torch.from_numpy(x), th, tw).permute(0, 2, 3, 1).numpy()
    cout = ref.shape[-1]
    assert (y[..., :cout] == ref).all() and (y[..., cout:] == 0).all()


def test_head_stencil_reference_by_hand():
    g = np.random.default_rng(5)
    img, k, bias = g.standard_normal((1, 3, 4, 5)), g.standard_normal((9, 5, 5, 3)), g.standard_normal(9)
    y = KR.head_stencil5x5(img, k, bias)
    for oy, ox, cs in [(0, 0, 0), (0, 2, 1), (0, 4, 2), (2, 0, 3), (1, 3, 4), (2, 4, 5), (3, 0, 6), (3, 1, 7), (3, 4, 8)]:
        acc = bias[cs]
        for fy in range(5):
            for fx in range(5):
                iy, ix = oy + fy - 2, ox + fx - 2
                if 0 <= iy < 4 and 0 <= ix < 5:
                    acc += (img[0, :, iy, ix] * k[cs, fy, fx]).sum()
        assert abs(y[0, oy, ox] - acc) < 1e-12


def test_patch_merge_gather_order():
    x = np.arange(2 * 3 * 3 * 1, dtype=np.float64).reshape(2, 3, 3, 1)
    rows = KR.patch_merge_gather(x)
    assert rows.shape == (8, 4)
    assert rows[0].tolist() == [0, 3, 1, 4]            # (0,0), (1,0), (0,1), (1,1)
    assert rows[3].tolist() == [8, 0, 0, 0]            # (2,2) and three tokens outside the odd map


needs_hipcc = pytest.mark.skipif(KH.hipcc() is None, reason="no hipcc")


@needs_hipcc
def test_harness_builds_and_wraps_every_launcher():
    so = ctypes.CDLL(KH.build())
    names = KH.launcher_names()
    assert len(names) >= 16 and "launch_layernorm" in names and "launch_head_stencil5x5" in names
    missing = [n for n in names if not hasattr(so, "kh_" + n)]
    assert not missing, f"launchers without a harness wrapper: {missing}"
    assert hasattr(so, "kh_gap_scratch_floats")
    assert sorted(KH.SIGNATURES) == names, "kernel_harness.SIGNATURES does not list the launchers of the two kernel files"


@needs_hipcc
def test_harness_object_name_follows_its_sources(monkeypatch):
    before = KH.object_path()
    monkeypatch.setattr(KH, "_flags", lambda: ["-O2"])
    assert KH.object_path() != before
