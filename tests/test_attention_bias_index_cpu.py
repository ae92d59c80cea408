"""csrc/kernels/window_attention_index.h on the CPU: the index into a head's REVERSED relative position bias column that the split and bf16
window attention kernels form — one address per 16-key tile (att_qrev + att_koff), four consecutive words from it.
tests/attention_bias_index_main.cpp is compiled around the header with the host compiler and checks, for every query token 0..143 and every
key 0..143, that the index lies in 0..528 and equals 528 - (att_qbase - key - 11 (key / 12)); and, for every window of every map up to
40 x 40 (padded rows / columns, shift 0 and 6, packed queries or not), that every query slot a workgroup can form — the slots past the last
real query are clamped to it — reads inside the table."""
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
    exe = str(tmp_path_factory.mktemp("attention_bias_index") / "attention_bias_index")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "attention_bias_index_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_every_query_key_pair_reads_its_table_word(report):
    assert report.splitlines()[-1] == "ok"
    m = re.search(r"^pairs (\d+) range (\d+) (\d+)$", report, re.M)
    assert m, report[-2000:]
    assert int(m.group(1)) == 144 * 144
    assert (int(m.group(2)), int(m.group(3))) == (0, 528)        # the whole table is used and nothing beyond it


def test_slots_past_the_last_real_query_stay_inside_the_table(report):
    m = re.search(r"^slots (\d+) past_nq (\d+)$", report, re.M)
    assert m, report[-2000:]
    assert int(m.group(1)) > 0 and int(m.group(2)) > 0           # padded windows with clamped slots were among the cases
