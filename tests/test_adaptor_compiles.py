"""include/cvo_adaptor.hpp -- the drop-in `cvo::cvo` for a box with the reference's dependencies -- against a compiler:
g++ -fsyntax-only with the stand-in Eigen / OpenCV / data_type.h declarations of tests/stubs/ (this image has neither
library), and its public interface diffed against the reference's class (thirdparty/cvo/include/cvo.hpp:216-276)."""
import json
import os
import re
import subprocess

from conftest import GOLDEN, ROOT

USE = os.path.join(ROOT, "tests", "cpp", "adaptor_use.cpp")


def test_adaptor_compiles_against_the_stand_in_headers():
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "tests", "stubs"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adaptor_use.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_every_public_member_of_the_reference_class_is_pinned():
    """tests/cpp/adaptor_use.cpp static_asserts the signature of each public member (the compile above is the diff).  The list of
    members it pins is checked to be complete against the reference's class, as recorded in tests/golden/reference_cvo_public_members.json
    (tests/golden/make_golden.py --reference): every function declared in the public section of cvo::cvo
    (thirdparty/cvo/include/cvo.hpp:213-281) and the public data members (cvo.hpp:137-144)."""
    pinned = set(re.findall(r"SAME\((\w+),", open(USE).read()))
    assert len(pinned) >= 19
    with open(os.path.join(GOLDEN, "reference_cvo_public_members.json")) as f:
        ref = json.load(f)
    declared = set(ref["functions"])
    assert declared and declared <= pinned, sorted(declared - pinned)
    for d in ("first_frame", "init", "iter", "transform", "prev_transform", "accum_transform"):
        assert d in ref["data_members"] and d in open(USE).read()
