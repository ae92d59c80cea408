"""csrc/kernels/window_attention_select.h on the CPU: the function that chooses the window attention kernel, its grid and block, or rejects the
parameters.  tests/attention_select_main.cpp is compiled around it with the host compiler under AddressSanitizer / UBSan and compares it with
the nested launcher code it replaced (restated there as it stood) over the full product of window side, planes, output form, fp16 planes,
storage type, C / heads, shift, BRN_ATT_HPW, BRN_ATT_F32_WAVES, diag build and twelve forms of the second map: every combination, none skipped."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "candle_birefnet_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("attention_select") / "attention_select")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "attention_select_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_selector_equals_the_nested_launcher_for_every_combination(report):
    assert report.splitlines()[-1] == "ok"


def test_both_valid_and_invalid_combinations_were_compared(report):
    m = re.search(r"^valid (\d+) invalid (\d+)$", report, re.M)
    assert m, report[-2000:]
    valid, invalid = int(m.group(1)), int(m.group(2))
    assert valid > 0 and invalid > 0
    assert valid + invalid == 4 * 3 * 3 * 2 * 2 * 3 * 6 * 3 * 2 * 2 * 2 * 12
