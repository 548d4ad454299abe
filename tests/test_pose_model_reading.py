"""tests/pose_model_reading.py (the dense numpy reading of the pose models) against central differences of the energy it differentiates, against
tests/hypothesis_reading.py for value and num, cvo_slam_amd.pose_model's two functions, and the plumbing of the three entry points that needs no GPU.

grad and hess must agree with central differences (step 1e-4, float64, the inside set frozen, the twist applied through helpers.se3_exp) to 1e-4 of
the largest entry.  What the reading gives: 6.5e-6 for grad and 3.3e-6 for hess at most; without S, or with -S, hess is off by 8.8e-4 to 1.1e-2 at
the two poses away from the optimum, nine bounds at least -- the test decides the sign of S."""
import os
import re
import subprocess

import numpy as np
import pytest

import hypothesis_reading as hr
import pose_model_reading as pm
from conftest import ROOT
from helpers import make_tf, se3_exp

BOUND = 1e-4
NEW_SYMBOLS = ["cvo_pose_models", "cvo_batch_pose_models", "cvo_batch_result_models"]
POSES = ["truth", "small", "mixed"]


def small_tf():
    return make_tf([0.2, 1, 0.1], 0.01, [0.004, -0.002, 0.003])


def pose_of(p, which):
    from cvo_slam_amd import hypotheses
    if which == "truth":
        return np.asarray(p.true_transform, np.float32)
    if which == "small":
        return hypotheses.compose(small_tf(), p.true_transform).astype(np.float32)
    return hr.hypothesis_set(p.true_transform)[14]                       # the "mixed" perturbation


def rel_err(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("which", POSES)
@pytest.mark.parametrize("ell", hr.ELLS)
@pytest.mark.parametrize("case", hr.CASES)
def test_reading_against_central_differences(case, ell, which):
    from cvo_slam_amd import synth
    p = synth.make_small_pair(*case)
    moving, fixed = (p.moving.xyz, p.moving.feat), (p.fixed.xyz, p.fixed.feat)
    T = pose_of(p, which)
    m = pm.model(moving, fixed, T, ell)
    value, num = hr.score(moving, fixed, T, ell)
    assert m["value"].tobytes() == value.tobytes() and m["num"] == num and num > 1
    grad, hess = pm.central_differences(pm.frozen_energy(moving, fixed, T, ell), 1e-4)
    eg, eh = rel_err(m["grad"], grad), rel_err(m["hess"], hess)
    e0 = rel_err(pm.model(moving, fixed, T, ell, with_s=0.0)["hess"], hess)
    em = rel_err(pm.model(moving, fixed, T, ell, with_s=-1.0)["hess"], hess)
    print(case, ell, which, "grad", eg, "hess", eh, "without S", e0, "with -S", em)
    assert np.array_equal(m["hess"], m["hess"].T)
    assert eg <= BOUND and eh <= BOUND
    if which != "truth":                                                 # away from the optimum a hess without S, or with -S, misses the bound
        assert e0 > BOUND and em > BOUND
    assert (np.abs(m["grad"]) <= m["mag_grad"]).all() and (np.abs(m["hess"]) <= m["mag_hess"]).all()


def test_float32_terms_against_float64_terms():
    """the reading's float32 terms against the same sums from float64 terms (the central differences' energy, differentiated by hand in double):
    far inside the GPU test's bound of 1e-6 of the magnitudes"""
    from cvo_slam_amd import synth
    p = synth.make_small_pair(31, 700)
    moving, fixed = (p.moving.xyz, p.moving.feat), (p.fixed.xyz, p.fixed.feat)
    T = pose_of(p, "mixed"); ell = 0.06
    m = pm.model(moving, fixed, T, ell)
    pa, pb, _, ck, _ = pm.inside_pairs(moving, fixed, T, ell)
    pa, pb = pa.astype(np.float64), pb.astype(np.float64)
    il2 = 1.0 / (np.float64(np.float32(ell)) ** 2)
    s2 = np.float64(np.float32(0.1) * np.float32(0.1))
    a = ck.astype(np.float64) * s2 * np.exp(-((pa - pb) ** 2).sum(axis=1) / (2.0 * ell * ell))
    w = il2 * a
    grad = np.concatenate([(w[:, None] * np.cross(pa, pb)).sum(axis=0), (w[:, None] * (pb - pa)).sum(axis=0)])
    worst = float((np.abs(m["grad"] - grad) / m["mag_grad"]).max())
    print("float32 against float64 terms, grad, in units of the magnitude:", worst)
    assert worst <= 1e-6                                                 # a term carries at most 16 float roundings of 2^-24: 9.5e-7 of its magnitude


def test_newton_step_and_retract():
    from cvo_slam_amd import pose_model
    rng = np.random.default_rng(3)
    A = rng.normal(size=(6, 6)); H = -(A @ A.T + np.eye(6)); g = rng.normal(size=6)
    d = pose_model.newton_step(g, H)
    np.testing.assert_allclose(-H @ d, g, atol=1e-12)
    d2 = pose_model.newton_step(g, H, damping=1e6)
    np.testing.assert_allclose(d2, g / 1e6, rtol=1e-4)
    T = make_tf([1, -2, 0.5], 0.3, [0.1, -0.2, 0.3])
    for delta in (np.array([0.3, -0.2, 0.5, 0.1, 0.2, -0.4]), np.array([1e-7, 2e-7, -1e-7, 0.01, 0.02, 0.03]), np.zeros(6)):
        E = se3_exp(delta[:3], delta[3:], 1.0)
        want = (E @ np.vstack([np.asarray(T, np.float64), [0, 0, 0, 1]]))[:3]
        got = pose_model.retract(delta, T)
        assert got.shape == (3, 4) and got.dtype == np.float64
        np.testing.assert_allclose(got, want, atol=1e-12)


def test_newton_step_raises_the_energy_on_the_reading():
    """the "mixed" start of each case and ell: hess is negative definite and one Newton step raises the energy (x1.2 to x6.4 on the reading)"""
    from cvo_slam_amd import pose_model, synth
    for case in hr.CASES:
        p = synth.make_small_pair(*case)
        moving, fixed = (p.moving.xyz, p.moving.feat), (p.fixed.xyz, p.fixed.feat)
        T = pose_of(p, "mixed")
        for ell in hr.ELLS:
            m = pm.model(moving, fixed, T, ell)
            assert np.linalg.eigvalsh(m["hess"]).max() < 0
            T1 = pose_model.retract(pose_model.newton_step(m["grad"], m["hess"]), T)
            v0, v1 = hr.score(moving, fixed, T, ell)[0], hr.score(moving, fixed, T1.astype(np.float32), ell)[0]
            print(case, ell, "value", float(v0), "->", float(v1), "x", float(v1) / float(v0))
            assert v1 > v0


def test_the_three_entry_points_are_declared_exported_and_bound(hiplib):
    src = open(os.path.join(ROOT, "include", "cvo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cvo_[a-zA-Z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", hiplib.lib_path()], text=True)
    exported = set(re.findall(r" T (cvo_[a-zA-Z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/cvo_hip.h"
        assert name in exported, f"{name} is not exported by the built library"
        assert name in hiplib.api.ABI_SYMBOLS, f"{name} is not listed in api.ABI_SYMBOLS"
    assert re.search(r"typedef\s+struct\s+cvo_pose_model\b", src)
    import ctypes
    assert ctypes.sizeof(hiplib.api.PoseModel) == 344
    for cls, name in ((hiplib.Cvo, "pose_models"), (hiplib.CvoBatch, "pose_models"), (hiplib.CvoBatch, "result_models")):
        assert callable(getattr(cls, name, None)), (cls.__name__, name)
