"""csrc/kernels/conv_halo_geometry.h on the CPU: the predicate that routes a launch to the halo-staged conv kernel and the kernel's tile <-> pixel
map.  tests/conv_halo_geometry_main.cpp is compiled around it with the host compiler under AddressSanitizer / UBSan and run directly: the map is
a bijection onto [0, M) for the test geometries and the model's map sizes, the predicate takes the model's twelve launches and refuses stride 2,
dilation 2, 7 x 7, Cin % 32 != 0 and three planes."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "candle_birefnet_amd", "csrc")


def test_geometry_and_predicate(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "conv_halo_geometry")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "conv_halo_geometry_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "ok"
