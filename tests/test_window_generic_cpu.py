"""csrc/kernels/window_generic_geometry.h on the CPU: the index math that the pack, bias-build and scatter kernels of the generic window
route (window sides other than 12 and 7) and their host path share.  tests/window_generic_main.cpp is compiled around it with the host
compiler under AddressSanitizer / UBSan and checks, for window sides 2, 3, 5, 8, 16, 24, 32, shift 0 and ws / 2, canvases of 1 x 1 to
4 x 5 windows with ragged H and W, and 1 and 3 images:
  (a) slot -> (image, wy, wx) is a bijection and its inverse agrees;
  (b) interior slots precede border slots, border = last window row or column, and a border slot's pattern is (slot - first) mod n_border;
  (c) against a brute-force three-slice region image (swin.rs:612-632): every interior window's mask is all zero, every border
      pattern equals the mask of its window;
  (d) the source index (roll + pad) and the destination index (un-roll + crop) round-trip over every real token exactly once."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "candle_birefnet_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("window_generic") / "window_generic")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "window_generic_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_slots_masks_and_round_trip_for_every_geometry(report):
    assert report.splitlines()[-1] == "ok"


def test_every_case_of_the_product_ran(report):
    """7 window sides x 2 shifts x (4 x 5 canvases) x 2 batch sizes x 9 ragged maps"""
    f = report.splitlines()[-2].split()
    assert f[0] == "cases" and int(f[1]) == 7 * 2 * 20 * 2 * 9 and int(f[3]) > 0
