"""The 16-bit weight layouts of csrc/brn_pack.h (what brn_weights.cpp uploads) against a numpy restatement of the documented layouts, at
the smallest shapes that exercise each layout rule.  The packers are pure host code: they are compiled with the host compiler into a
stand-alone program under AddressSanitizer / UBSan and run directly (no GPU, no HIP).  Every comparison is exact equality of integers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("weight_pack")
    exe = str(d / "weight_pack")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "candle_birefnet_amd", "csrc"), os.path.join(ROOT, "tests", "weight_pack_main.cpp"), "-o", exe])

    def run(what, x, *ints):
        src, dst = str(d / "in.f32"), str(d / "out.u16")
        np.ascontiguousarray(x, np.float32).tofile(src)
        subprocess.check_call([exe, what, src, dst] + [str(int(i)) for i in ints])
        return np.fromfile(dst, np.uint16)
    return run


def weights(shape, seed, scale=0.05):
    """values over many binades, with exact zeros, ties of the bf16 rounding and both signs"""
    r = np.random.default_rng(seed)
    w = (r.standard_normal(shape) * scale * np.exp2(r.integers(-6, 3, shape))).astype(np.float32)
    flat = w.reshape(-1)
    flat[::17] = 0.0
    flat[5::29] = np.float32(1.0 + 2.0 ** -8)          # a tie of fp32 -> bf16 (to even: down)
    flat[7::31] = np.float32(-(1.0 + 3 * 2.0 ** -8))   # a tie (to even: up)
    return w


def bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_f32(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def s16(x, f16):
    return np.asarray(x, np.float32).astype(np.float16).view(np.uint16) if f16 else bf16(x)


@pytest.mark.parametrize("nplanes", [2, 3])
def test_bf16_planes(packer, nplanes):
    N, K = 128, 64
    w = weights((N, K), 1)
    got = packer("planes", w, K, nplanes).reshape(N, K // 32, nplanes, 32)        # [row][K/32][plane][32]
    r = w.copy()
    for p in range(nplanes):                                                   # plane p = RN_bf16(x - the planes before it)
        h = bf16(r)
        assert np.array_equal(got[:, :, p, :].reshape(N, K), h), p
        r = r - bf16_f32(h)
    assert np.count_nonzero(got[:, :, 1, :]) > N * K // 2                      # the second plane carries something


def test_half2_planes_and_scale(packer):
    N, K = 128, 64
    w = weights((N, K), 2)
    out = packer("half2", w, K)
    sc = out[-2:].view(np.float32)[0]
    mx = np.abs(w).max()
    assert sc == np.float32(2.0) ** (14 - np.frexp(mx)[1]) and 2.0 ** 13 <= mx * sc < 2.0 ** 14
    got = out[:-2].reshape(N, K // 32, 2, 32)
    x = w * sc                                                                  # (a power of two: exact)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    assert np.array_equal(got[:, :, 0, :].reshape(N, K), hi.view(np.uint16))
    assert np.array_equal(got[:, :, 1, :].reshape(N, K), lo.view(np.uint16))


@pytest.mark.parametrize("f16", [0, 1])
def test_s16_storage_dense_pads_rows_to_256_and_k_to_64(packer, f16):
    N, K = 130, 96
    w = weights((N, K), 3)
    out = packer("s16", w, K, f16, 0, K)
    assert list(out[-3:]) == [256, 128, 0]                                      # rows, ld, chunk_major
    want = np.zeros((256, 128), np.uint16)
    want[:N, :K] = s16(w, f16)
    assert np.array_equal(out[:-3].reshape(256, 128), want)


@pytest.mark.parametrize("cinp,chunk_major", [(128, 1), (64, 0)])
def test_s16_storage_conv(packer, cinp, chunk_major):
    O, taps = 16, 9
    K = taps * cinp
    pk = weights((O, taps, cinp), 4)                                            # the packed conv matrix: K order (tap, channel)
    out = packer("s16", pk, K, 0, taps, cinp)
    assert list(out[-3:]) == [256, K, chunk_major]
    if chunk_major:                                                             # K order (64-channel chunk, tap, channel in chunk)
        src = pk.reshape(O, taps, cinp // 64, 64).transpose(0, 2, 1, 3)
    else:
        src = pk
    want = np.zeros((256, K), np.uint16)
    want[:O] = bf16(src.reshape(O, K))
    assert np.array_equal(out[:-3].reshape(256, K), want)
    # a dense matrix of the same shape is never reordered
    assert packer("s16", pk, K, 0, 0, cinp)[-1] == 0


def frag_lane(k, n):
    return ((k >> 3) & 3) * 16 + (n & 15)


def test_dense_frags(packer):
    N, K = 192, 192
    w = weights((N, K), 5)
    got = packer("dense", w, N, K, 0).reshape(N // 16, K // 32, 64, 8)           # [n / 16][K / 32][lane][8]
    want = np.zeros_like(got)
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    want[n >> 4, k >> 5, frag_lane(k, n), k & 7] = bf16(w)
    assert np.array_equal(got, want)


def test_deform_frags(packer):
    N, Cin, Cinp, taps = 16, 40, 64, 9
    w = weights((N, Cin, taps), 6)                                              # candle's [O][Cin][kh kw]
    got = packer("deform", w, N, Cin, Cinp, taps, 1).reshape(256 // 16, taps * Cinp // 64, 2, 64, 8)   # [n / 16][K / 64][k32 half][lane][8]
    want = np.zeros_like(got)
    n, ci, t = np.meshgrid(np.arange(N), np.arange(Cin), np.arange(taps), indexing="ij")
    k = t * Cinp + ci                                                           # K order (tap, channel), channels padded to Cinp
    want[n >> 4, k >> 6, (k >> 5) & 1, frag_lane(k, n), k & 7] = s16(w, True)
    assert np.array_equal(got, want)
    assert not got[1:].any() and np.count_nonzero(got) > N * Cin * taps * 3 // 4   # rows 16 .. 255 and the pad channels stay zero
