"""The plane-exact data of conv_halo_cases.py on the CPU: every case's im2col rows stay within gemm_cases.NNZ non-zeros and satisfy
kernel_refs.assert_plane_exact, so test_conv_halo_gpu.py may ask for bit-for-bit equality with the fp64 reference; and the case list holds
what it is meant to hold."""
import numpy as np
import pytest

import conv_halo_cases as HC
import kernel_refs as KR


@pytest.mark.parametrize("case", HC.CASES, ids=lambda c: c.id)
def test_plane_exact_condition(case):
    assert 0 < HC.exactness_margin(case) < 1


@pytest.mark.parametrize("case", HC.CASES, ids=lambda c: c.id)
def test_reference_is_exact_in_fp32_and_not_trivial(case):
    ref = HC.host(case, True)["ref"]
    assert (ref.astype(np.float32).astype(np.float64) == ref).all()
    assert np.count_nonzero(ref) > ref.size // 4


def test_case_list_covers_what_it_claims():
    cs = HC.CASES
    assert {c.form for c in cs} == {"h2", "bf16x2"} and {c.cfg for c in cs} == {1, 2}
    assert {(c.form, c.cfg) for c in cs} == {(f, g) for f in ("h2", "bf16x2") for g in (1, 2)}
    assert {c.N for c in cs} == {64, 16, 50} and {c.geo for c in cs} == set(HC.GEOMETRIES)
    assert any(c.bias and c.scale and c.act == KR.ACT_RELU for c in cs) and any(c.c_coff and c.c_pad for c in cs) and any(c.R for c in cs)
    B, H, W, Cin, ld, coff = HC.GEOMETRIES["wide"]
    assert B == 2 and H % 8 and W % 16 and H > 8 and W > 16 and Cin == 64 and (ld, coff) == (128, 32)
    B, H, W, Cin, ld, coff = HC.GEOMETRIES["small"]
    assert H < 8 and W < 16
    assert HC.GEOMETRIES["uneven"][3] // 32 == 3 and HC.SPLITK["uneven"] == 2        # slices of 2 chunks and 1 chunk
    assert HC.GEOMETRIES["empty"][3] // 32 == 2 and HC.SPLITK["empty"] == 3          # slices of 1, 1 and 0 chunks
