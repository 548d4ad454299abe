"""The "Eigen 3.3.7" arithmetic mode on the host (no GPU): the public header's declarations and constants, the mode's two epilogue
pieces (cvo_slam_amd/csrc/cvo_eigen337.hpp) built alone with g++ and compared bit for bit with the oracle's variants, and the adaptor's
extra member against the stand-in headers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import arith_cases

HEADER = os.path.join(ROOT, "include", "cvo_hip.h")
CSRC = os.path.join(ROOT, "cvo_slam_amd", "csrc")


def _enum(path, prefix):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(" + prefix + r"[A-Z0-9_]+)\s*=\s*([^,}]+)", src)}


def test_header_declares_the_mode():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for sig in (r"int\s+cvo_set_arith_mode\s*\(\s*cvo_handle\s+h\s*,\s*int\s+flags\s*\)",
                r"int\s+cvo_get_arith_mode\s*\(\s*cvo_handle\s+h\s*,\s*int\s*\*\s*flags\s*\)",
                r"int\s+cvo_batch_set_arith_mode\s*\(\s*cvo_batch\s+b\s*,\s*int\s+flags\s*\)",
                r"int\s+cvo_batch_get_arith_mode\s*\(\s*cvo_batch\s+b\s*,\s*int\s*\*\s*flags\s*\)",
                r"int\s+cvo_selftest_cubic_step_f32eig\s*\(\s*int\s+device\s*,\s*int\s+n\s*,\s*const\s+float\s*\*\s*coef_minstep\s*,\s*float\s*\*\s*step_out\s*\)",
                r"int\s+cvo_selftest_dist_se3_f32logm\s*\(\s*int\s+device\s*,\s*int\s+n\s*,\s*const\s+float\s*\*\s*dR_dT\s*,\s*float\s*\*\s*dist_out\s*\)"):
        assert re.search(sig, src), sig


def test_mode_bits_are_the_oracle_variant_bits():
    cvo = {k: eval(v.replace("|", " | ")) for k, v in _enum(HEADER, "CVO_ARITH_").items()}
    orc = {k: int(v) for k, v in _enum(os.path.join(ROOT, "oracle", "cvo_oracle.h"), "ORC_VAR_").items()}
    assert cvo == {"CVO_ARITH_BASE": 0, "CVO_ARITH_F32_ROOTS": 2, "CVO_ARITH_F32_LOGM": 4, "CVO_ARITH_ROW_LAZY16": 8, "CVO_ARITH_EIGEN337": 14}
    for name in ("F32_ROOTS", "F32_LOGM", "ROW_LAZY16"):
        assert cvo["CVO_ARITH_" + name] == orc["ORC_VAR_" + name]
    assert cvo["CVO_ARITH_EIGEN337"] == orc["ORC_VAR_F32_ROOTS"] | orc["ORC_VAR_F32_LOGM"] | orc["ORC_VAR_ROW_LAZY16"]
    from cvo_slam_amd import api
    assert (api.ARITH_BASE, api.ARITH_F32_ROOTS, api.ARITH_F32_LOGM, api.ARITH_ROW_LAZY16, api.ARITH_EIGEN337) == (0, 2, 4, 8, 14)
    assert api.arith_flags("base") == 0 and api.arith_flags("eigen337") == 14 and api.arith_flags(8) == 8
    with pytest.raises(ValueError):
        api.arith_flags("eigen")


WRAP = r"""
#include "cvo_eigen337.hpp"
extern "C" void many_cubic(int n, const float* in, float* out) {
    for (int i = 0; i < n; ++i) out[i] = cvohip::cubic_step_f32eig(in[5 * i], in[5 * i + 1], in[5 * i + 2], in[5 * i + 3], in[5 * i + 4]);
}
extern "C" void many_dist(int n, const float* in, float* out) {
    for (int i = 0; i < n; ++i) out[i] = cvohip::dist_se3_f32logm(in + 12 * i, in + 12 * i + 9);
}
"""


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("e337")
    src, so = d / "wrap.cpp", d / "libe337.so"
    src.write_text(WRAP)
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + CSRC, str(src), "-o", str(so)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(str(so))
    fp = C.POINTER(C.c_float)
    for name in ("many_cubic", "many_dist"):
        getattr(L, name).argtypes = [C.c_int, fp, fp]
    return L


def _run(L, name, a, width):
    a = np.ascontiguousarray(a, np.float32).reshape(-1, width); out = np.zeros(a.shape[0], np.float32)
    fp = C.POINTER(C.c_float)
    getattr(L, name)(a.shape[0], a.ctypes.data_as(fp), out.ctypes.data_as(fp))
    return out


def test_cubic_step_f32eig_equals_the_oracle(host_lib, oracle):
    cases = arith_cases.cubic_cases()
    assert len(cases) >= 100_000
    got = _run(host_lib, "many_cubic", cases, 5)
    want = np.array([oracle.cubic_step_f32eig(*map(float, c)) for c in cases], np.float32)
    bad = np.nonzero(arith_cases.bits(got) != arith_cases.bits(want))[0]
    assert bad.size == 0, (bad.size, cases[bad[:5]], got[bad[:5]], want[bad[:5]])
    # the cases do reach every exit: min_step, the clamp, roots in between, and answers that differ from the closed form's
    assert np.sum(want == np.float32(0.8)) > 1000 and np.sum(want == cases[:, 4]) > 1000 and np.sum((want < 0.8) & (want != cases[:, 4])) > 10000
    closed = np.array([oracle.cubic_step(*map(float, c)) for c in cases[:5000]], np.float32)
    assert np.any(closed != want[:5000])


def test_dist_se3_f32logm_equals_the_oracle(host_lib, oracle):
    cases = arith_cases.dist_cases(oracle)
    assert len(cases) >= 100_000
    got = _run(host_lib, "many_dist", cases, 12)
    want = np.array([oracle.dist_se3_f32logm(c[:9].reshape(3, 3), c[9:]) for c in cases], np.float32)
    bad = np.nonzero(arith_cases.bits(got) != arith_cases.bits(want))[0]
    assert bad.size == 0, (bad.size, cases[bad[:3]], got[bad[:3]], want[bad[:3]])
    assert want[0] == 0.0 and np.all(np.isfinite(want))


def test_adaptor_compiles_with_the_mode_member(tmp_path):
    """include/cvo_adaptor.hpp's set_arith_mode (not a member of the reference's class) against the stand-in headers, as
    tests/test_adaptor_compiles.py compiles the rest."""
    use = tmp_path / "adaptor_arith_use.cpp"
    use.write_text('#include "cvo_adaptor.hpp"\n'
                   "static_assert(std::is_same<decltype(&cvo::cvo::set_arith_mode), void (cvo::cvo::*)(int)>::value, \"set_arith_mode(int)\");\n"
                   "void use_mode(cvo::cvo& c) { c.set_arith_mode(CVO_ARITH_EIGEN337); c.set_arith_mode(CVO_ARITH_BASE); }\n")
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "tests", "stubs"), "-I" + os.path.join(ROOT, "include"), str(use)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
