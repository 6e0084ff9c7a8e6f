"""The all-or-none rule of the op kernels (euler_amd/csrc/op_framework.cc: OpOutputs): on every return
from Compute either all outputs of the op are in the context, or none of the names the invocation
created is.  tests/csrc/op_rollback_check.cc drives the kernels through CreateOpKernel / Compute with one
output name already taken by the caller - Allocate / AddAlias then fail, no device error is involved -
and exits non-zero on the first violated check.  The Download / Sync failure paths need a device error
and are not driven; they leave through the same destructor."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe():
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "op_rollback_check")
    src = os.path.join(HERE, "csrc", "op_rollback_check.cc")
    lib = os.path.join(ROOT, "euler_amd", "lib", "libeuler_gpu.so")
    deps = [src, lib] + [os.path.join(ROOT, "include", h) for h in ("euler_op_framework.h", "euler_gpu.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        # (linked the way examples/cpp/Makefile links its programs)
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        subprocess.check_call([hipcc, "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src,
                               "-L" + os.path.dirname(lib), "-leuler_gpu", "-lpthread",
                               "-Wl,-rpath,$ORIGIN/../../../euler_amd/lib", "-o", exe])
    return exe


def test_host_only_ops_roll_back(exe):
    """API_SPARSE_GEN_ADJ and API_GATHER_RESULT (no device work): a taken output name or a missing input
    leaves no output and no alias, the inputs stay reachable, every tensor is freed once; where there
    is no device, ID_UNIQUE logs and leaves no output."""
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host-only ops ok" in r.stdout, r.stdout
    assert r.stderr.count("Allocate output tensor failed!") == 2, r.stderr
    assert "API_GATHER_RESULT: missing input" in r.stderr, r.stderr
    if "no device" in r.stdout:
        assert "ERROR ID_UNIQUE" in r.stderr, r.stderr


@pytest.mark.gpu
def test_ops_publish_all_outputs_or_none(torch_cuda, exe):
    """Every case of the program on a 300-node synthetic graph: ID_UNIQUE (also with pinned 32 KB
    outputs, whose block serves the next run), IDX_GATHER, DATA_GATHER, API_GET_NB_NODE, API_SAMPLE_NB
    with and without post-process, API_GET_EDGE_SUM_WEIGHT, API_SAMPLE_L and the host-only ops."""
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all ops ok" in r.stdout, r.stdout
    # 2 host-only collisions, ID_UNIQUE twice, the two gathers, GET_NB, SAMPLE_NB twice, SUM_WEIGHT, SAMPLE_L
    assert r.stderr.count("Allocate output tensor failed!") == 11, r.stderr
