"""The launch sequence of the forward graph (csrc/brn_graph*.cpp) against a recorded one, on the CPU.  The graph sources are compiled with the
host compiler, under AddressSanitizer / UBSan, against stubs that log every kernel launch and HIP runtime call with all its arguments
(tests/graph_trace_stubs.cpp); tests/graph_trace_main.cpp runs descriptor-only models in every compute mode and both deform modes through
them.  The log must equal tests/golden/graph_trace_*.txt.gz (gzip of the text, 0.55 MB each unpacked) exactly: enqueue order, stream of
every launch, arena offsets, every field of every launched descriptor, the profiling records.  The golden files record what the host code launched before it was restructured; they
change only when a change of the launch sequence is intended."""
import difflib
import glob
import gzip
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "candle_birefnet_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

# the other side of every switch the graph reads (csrc/brn_host.h, struct Switches)
SWITCHED = {"BRN_WSTAT": "0", "BRN_WSTAT_LN": "0", "BRN_ROWLN": "3", "BRN_PATCH_LN": "0", "BRN_P1_F32": "0", "BRN_H2_ATT": "0",
            "BRN_DEFORM_F32_KERNEL": "1"}


@pytest.fixture(scope="module")
def tracer(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("graph_trace") / "graph_trace")
    graph = sorted(glob.glob(os.path.join(CSRC, "brn_graph*.cpp")))
    assert graph, "no graph sources"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                           os.path.join(ROOT, "tests", "graph_trace_main.cpp"), os.path.join(ROOT, "tests", "graph_trace_stubs.cpp")] + graph +
                          ["-o", exe])

    def run(extra_env):
        env = {k: v for k, v in os.environ.items() if not k.startswith("BRN_")}
        env.update(extra_env)
        r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout
    return run


def check(got, golden):
    with gzip.open(os.path.join(ROOT, "tests", "golden", golden + ".gz"), "rt") as f:
        want = f.read()
    if got == want:
        return
    diff = [ln for ln in difflib.unified_diff(want.splitlines(), got.splitlines(), golden, "this build", lineterm="", n=1)]
    changed = [i for i, ln in enumerate(diff) if ln[:1] in "+-" and ln[:3] not in ("+++", "---")]
    last = changed[39] if len(changed) > 40 else len(diff) - 1
    pytest.fail("the launch trace differs from %s (%d differing lines):\n%s" % (golden, len(changed), "\n".join(diff[:last + 1])), pytrace=False)


def test_launch_trace_default_switches(tracer):
    check(tracer({}), "graph_trace_default.txt")


def test_launch_trace_switched(tracer):
    check(tracer(SWITCHED), "graph_trace_switched.txt")
