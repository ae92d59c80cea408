"""The case table and references of gemm_s16_cases.py, checked without a GPU: every exact case meets its exactness conditions in both storage
types, exact ties of the 16-bit conversion occur, the GELU arguments stay within |x| <= 6, the persistent walk of gemm_bf16_kernel (restated)
visits every work item of every case once and gives every workgroup of the walk cases three or more items, and — through the product's own
planner — which tile every shape of test_linear_bf16_mode / test_conv2d_bf16_mode runs on: the coverage gap test_gemm_s16_forms_gpu.py closes,
as a checked fact.  Where hipcc is present, the 16-bit GEMM harness builds beside the other two."""
import ctypes
import os

import numpy as np
import pytest

import gemm_harness as GH32
import gemm_s16_cases as GC
import gemm_s16_harness as GH
import kernel_harness as KH
import kernel_refs as KR

S16 = ["bf16", "f16"]


def test_case_ids_are_unique_and_the_table_is_small():
    ids = [c.id for c in GC.ALL_CASES]
    assert len(set(ids)) == len(ids)
    assert len(ids) <= 230


@pytest.mark.parametrize("s16", S16)
@pytest.mark.parametrize("case", GC.ALL_CASES, ids=lambda c: c.id)
def test_exactness_conditions_hold(case, s16):
    assert 0 < GC.assert_exact(case, s16) <= 16 * case.K
    if case.act == KR.ACT_GELU:                            # the Gaussian run's arguments too
        assert np.abs(GC.host(case, s16, False)["pre"]).max() <= 6


@pytest.mark.parametrize("s16,above", [("bf16", 256), ("f16", 2048)])
def test_exact_ties_of_the_conversion_occur(s16, above):
    """integer results above 256 (bf16) / 2048 (fp16) that lie halfway between two 16-bit numbers: the tie rule of the conversion is tested"""
    n = 0
    for case in GC.TILE_CASES:
        if case.positive:
            ref = GC.host(case, s16, True)["ref"]
            assert np.abs(ref).max() > above
            n += GC.ties(ref, s16)
    assert n > 1000
    walk = GC.host(GC.WALK_CASES[12], s16, True)["ref"]    # a signed K = 256 case: bf16 ties without the unsigned data
    assert GC.WALK_CASES[12].K == 256 and (GC.ties(walk, "bf16") > 100)


def test_16_bit_helpers():
    x = np.array([1.0, 1.5, 257.0, 2049.0, -2049.0, 3e-6, 0.0])
    assert GC.ulp16(x, "bf16").tolist() == [2.0 ** -7, 2.0 ** -7, 2.0, 16.0, 16.0, 2.0 ** -26, 2.0 ** -133]
    assert GC.ulp16(x, "f16").tolist() == [2.0 ** -10, 2.0 ** -10, 0.25, 2.0, 2.0, 2.0 ** -24, 2.0 ** -24]
    assert GC.floor16(x, "bf16")[2:5].tolist() == [256.0, 2048.0, -2064.0] and GC.ceil16(x, "bf16")[2:5].tolist() == [258.0, 2064.0, -2048.0]
    assert GC.ties(np.array([257.0, 258.0, 2049.0, 2056.0]), "bf16") == 2 and GC.ties(np.array([257.0, 2049.0, 2051.0, 2050.0]), "f16") == 2
    v, b = GC.to_s16(np.array([257.0, 259.0, 2049.0, 2051.0]), "bf16")            # ties go to the even mantissa
    assert v.tolist() == [256.0, 260.0, 2048.0, 2048.0] and b.tolist() == [0x4380, 0x4382, 0x4500, 0x4500]
    assert GC.to_s16(np.array([2049.0, 2051.0]), "f16")[0].tolist() == [2048.0, 2052.0]


@pytest.mark.parametrize("case", GC.ALL_CASES, ids=lambda c: c.id)
def test_walk_visits_every_item_once(case):
    per_wg, total = GC.walk(case)
    seen = sorted(i for w in per_wg for i in w)
    assert seen == list(range(total))
    BM, BN = case.tile
    tm, tn = -(-case.M // BM), -(-case.N // BN)
    assert sorted(GC.tile_coords(t, tm, tn) for t in range(tm * tn)) == [(i, j) for i in range(tm) for j in range(tn)]


def test_walk_cases_give_every_workgroup_three_items():
    """a condition on the case table: on a grid of 8 CUs every workgroup hands over twice or more, from full tiles to full and to ragged ones"""
    for case in GC.WALK_CASES[:GC.WALK_MAIN]:
        per_wg, total = GC.walk(case)
        assert case.cus == 8 and len(per_wg) == 8 * GC.WG_PER_CU[case.cfg]
        assert min(len(w) for w in per_wg) >= 3, case.id
        BM, BN = case.tile
        tm, tn = -(-case.M // BM), -(-case.N // BN)
        assert case.M % BM and case.N % BN                                   # a ragged last row tile and a ragged last column tile
        full = lambda t: (lambda i, j: i < tm - 1 and j < tn - 1)(*GC.tile_coords(t, tm, tn))          # noqa: E731
        pairs = {(full(a), full(b)) for w in per_wg for a, b in zip(w, w[1:])}
        assert {(True, True), (True, False)} <= pairs, case.id               # the counted wait after a full tile; the plain one after a ragged tile
    totals = [GC.walk(c)[1] for c in GC.WALK_CASES[GC.WALK_MAIN:]]
    assert totals == [20, 25, 45, 66, 6, 6, 6, 6]
    wide = [c for c in GC.WALK_CASES if -(-c.N // c.tile[1]) > 8]             # wider than tile_coords' groups of 8 tile columns
    assert {c.cfg for c in wide} == {0, 1}
    assert {(c.cfg, c.K) for c in GC.WALK_CASES[:GC.WALK_MAIN]} >= {(cfg, K) for cfg in range(4) for K in (64, 128, 192, 256)}


def test_flavours_and_tiles_are_all_forced():
    seen = {(c.cfg, c.flavour, bool(c.conv)) for c in GC.ALL_CASES}
    assert {(cfg, fl, conv) for cfg in range(4) for fl in (0, 1, 2, 3) for conv in (False, True)} - seen <= {(3, 3, True), (0, 3, True), (1, 1, True), (3, 1, True)}
    assert {c.flavour for c in GC.EPILOGUE_CASES if c.cfg == 2} == {0, 1, 2} == {c.flavour for c in GC.EPILOGUE_CASES if c.cfg == 0}
    assert all(c.tile == (128, 128) and c.K % 64 == 32 for c in GC.KTAIL_CASES)


def _shapes(fn, names):
    return [m.args[1] for m in fn.pytestmark if m.name == "parametrize" and m.args[0] == names][0]


SLOTS = {0: 512, 1: 768, 2: 256, 3: 256}


def test_planner_picks_for_the_op_level_tests():
    """plan_gemm_bf16 on every shape of test_linear_bf16_mode and test_conv2d_bf16_mode: the 256 x 256 tile is never planned, the implicit-GEMM
    form only meets the 128 x 64 tile, and no launch has more work items than persistent workgroups (no workgroup walks a second item)"""
    import test_ops_gpu as T
    lin, conv = [], []
    for M, K, N in _shapes(T.test_linear_bf16_mode, "M,K,N"):
        for gelu in (False, True):
            cfg, sk = GH.plan(M, N, K, True, gelu)                           # (the linear entry keeps y and the residual fp32)
            BM, BN = GC.TILES[cfg]
            lin.append((cfg, sk))
            assert -(-M // BM) * -(-N // BN) * sk <= SLOTS[cfg]
    for B, C, H, W, O, k, p in _shapes(T.test_conv2d_bf16_mode, "B,C,H,W,O,k,p"):
        M, K = B * H * W, k * k * C
        cfg, sk = GH.plan(M, O, K)
        BM, BN = GC.TILES[cfg]
        conv.append(cfg)
        assert -(-M // BM) * -(-O // BN) * sk <= SLOTS[cfg]
    assert len(lin) == 18 and len(conv) == 12
    assert lin[::2] == lin[1::2]                                             # the GELU hint changes nothing at these shapes
    assert [c for c, _ in lin[::2]] == [1, 1, 1, 1, 0, 1, 1, 1, 3] and all(sk == 1 for _, sk in lin)
    assert conv == [1] * 12
    M, K, N = _shapes(T.test_linear_bf16_mode, "M,K,N")[8]
    assert -(-M // 256) * -(-N // 192) == 129


def test_pack_s16_is_the_layout_the_cases_assume():
    """kh_pack_s16 = pack_s16_storage: RNE words, rows padded to 256, K to 64; Cin = 128 convs chunk-major (chunk, tap, channel in chunk)"""
    g = np.random.default_rng(3)
    for s16, (f16, _) in GC.S16.items():
        w = g.standard_normal((130, 96)).astype(np.float32)
        out, cm = GH.pack_host(w, f16)
        assert out.shape == (256, 128) and not cm and (out[:130, :96] == GC.to_s16(w, s16)[1]).all() and not out[130:].any() and not out[:, 96:].any()
        w = g.standard_normal((8, 9 * 128)).astype(np.float32)
        out, cm = GH.pack_host(w, f16, 9, 128)
        want = GC.to_s16(w, s16)[1].reshape(8, 9, 2, 64).transpose(0, 2, 1, 3).reshape(8, -1)
        assert cm and out.shape == (256, 1152) and (out[:8] == want).all()
        assert not GH.pack_host(w, f16, 0, 0)[1] and not GH.pack_host(w[:, :9 * 64], f16, 9, 64)[1]


needs_hipcc = pytest.mark.skipif(KH.hipcc() is None, reason="no hipcc")


@needs_hipcc
def test_gemm_s16_harness_builds_beside_the_other_two():
    so = ctypes.CDLL(GH.build())
    assert all(hasattr(so, n) for n in ["kh_launch_gemm_s16", "kh_pack_s16", "kh_plan_gemm_s16"])
    dirs = {os.path.dirname(p) for p in [GH.object_path(), GH32.object_path(), KH.object_path()]}
    assert len(dirs) == 3 and os.path.basename(GH.object_path()).startswith("gemm_s16_harness_")
    assert any(f.endswith("gemm_bf16.hip") for f in KH._with_headers(GH.SOURCES[2:]))        # the fp16 build is hashed through its include
