"""BatchLCQProblem::getJacobian, SubsolverHIP::getJacobian and the `blocked` argument of getSensitivity (lcqpow_amd/csrc/host) through a
C++ program of their own, tests/cpp/jacobian_test.cpp, compiled here against include/, the host library and liblcqpow_hip.so."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import __graft_entry__ as g
    g.build_hip(); g.build_host()
    out = str(tmp_path_factory.mktemp("jacobian_cpp") / "jacobian_test")
    libdir = os.path.join(ROOT, "lcqpow_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "csrc", "host"), "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "jacobian_test.cpp"), "-L", libdir, "-llcqpow_host", "-llcqpow_hip", "-Wl,-rpath," + libdir])
    return out


def test_jacobian_and_blocked_flag_from_cpp(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr
