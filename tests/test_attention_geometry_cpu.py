"""csrc/kernels/window_geometry.h on the CPU: the header the window attention kernels and their launcher share.  tests/attention_geometry_main.cpp
is compiled around it with the host compiler under AddressSanitizer / UBSan and checks, for every H, W in 1 .. 40 and shift 0 / 6: the query
slots of every window are a bijection (row-major) onto exactly the tokens whose brute-force tok_src is >= 0, nq is their count, the unpacked
form is the identity; the dispatch order of a one- and a two-geometry launch is a permutation of its windows with non-increasing tile
counts, and the identity where nothing is padded.  It prints the tile totals of the four stage geometries of a 1024 x 1024 image."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "candle_birefnet_amd", "csrc")

# (stage, shift) -> (windows of the full- and half-scale map, 16-query tiles over all positions, over the real queries only)
STAGE_TILES = {
    (0, 0): (605, 5445, 5120), (0, 6): (605, 5445, 5162),
    (1, 0): (157, 1413, 1280), (1, 6): (157, 1413, 1290),
    (2, 0): (45, 405, 320), (2, 6): (45, 405, 330),
    (3, 0): (13, 117, 80), (3, 6): (13, 117, 82),
}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("attention_geometry") / "attention_geometry")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "attention_geometry_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_slots_and_order_for_every_small_geometry(report):
    assert report.splitlines()[-1] == "ok"


def test_stage_tile_totals_of_the_flagship_geometry(report):
    got = {}
    for ln in report.splitlines():
        f = ln.split()
        if f and f[0] == "stage":
            got[(int(f[1]), int(f[3]))] = (int(f[5]), int(f[7]), int(f[9]))
    assert got == STAGE_TILES
