"""CPU checks of the reachability classes (cls_reach_classes_host, the
device-free twin of cls_reach_classes; vpp_amd.engine.expand_classes): the
classes, representatives, sizes, diagonal and quotient equal the definition's
direct restatement (reach_classes_cases.classes_ref) on every synthetic matrix
and on the oracle's two 37 x 3 matrices, the summary expands to the matrix
again, the numbering is canonical, a class_cap too small leaves the per-class
outputs alone, truncated keys (key_bits) give the same classes through more
rounds and no keys at all do not converge, every refusal leaves its outputs
alone; the boundary of cls_reach_classes itself (null arguments, the structure's
layout, the exported symbols, the classes_key_bits option), the Go shims'
C99 build and the Go binding's Go 1.9 API."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reach_cases as rc
import reach_classes_cases as cc
from vpp_amd import _abi
from vpp_amd.engine import expand_classes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "go", "contivcls", "contivcls.go")
SENTINEL = 0xA5
FIELDS = ["class_out", "n_classes", "class_cap", "rep_out", "size_out", "self_out", "quot_out", "verdict_out",
          "rounds", "sums_out"]


class Host:
    """cls_reach_classes_host on sentinel-filled outputs with room for cap classes."""

    def __init__(self, m, cap=None):
        self.m = np.ascontiguousarray(m)
        self.P, self.N, _ = P, N, _ = self.m.shape
        self.cap = cap = N if cap is None else cap
        self.out = dict(class_out=np.zeros(N, np.uint32), n_classes=np.zeros(1, np.uint32),
                        rep_out=np.zeros(max(cap, 1), np.uint32), size_out=np.zeros(max(cap, 1), np.uint32),
                        self_out=np.zeros(P * max(cap, 1), np.uint8), quot_out=np.zeros(P * max(cap, 1) ** 2, np.uint8),
                        verdict_out=np.zeros((P, N, N), np.uint8), rounds=np.zeros(1, np.uint32),
                        sums_out=np.zeros((P, N, 2), np.uint64))
        self.fill()

    def fill(self):
        for a in self.out.values():
            a.view(np.uint8).reshape(-1)[:] = SENTINEL

    def untouched(self, *names):
        return all((self.out[k].view(np.uint8) == SENTINEL).all() for k in (names or self.out))

    def call(self, key_bits=64, matrix=True, N=None, P=None, out=True, cap=None, **ptrs):
        o = {k: v.ctypes.data for k, v in self.out.items()}
        o["class_cap"] = self.cap if cap is None else cap
        o.update(ptrs)
        st = _abi.ReachClassesOut(*[o[k] for k in FIELDS])
        return _abi.lib().cls_reach_classes_host(self.m.ctypes.data if matrix else None, self.N if N is None else N,
                                                 self.P if P is None else P, key_bits, C.byref(st) if out else None)

    def result(self):
        """(classes, reps, sizes, self, quot) as classes_ref returns them."""
        c, P = int(self.out["n_classes"][0]), self.P
        return (self.out["class_out"], self.out["rep_out"][:c], self.out["size_out"][:c],
                self.out["self_out"][:P * c].reshape(P, c), self.out["quot_out"][:P * c * c].reshape(P, c, c))


def check(got, want, m, what):
    for name, g, w in zip(("classes", "reps", "sizes", "self", "quot"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), (what, name)
    classes, reps, sizes, self_, quot = got
    # canonical numbering: by ascending smallest member
    assert classes[0] == 0 and (np.diff(reps.astype(np.int64)) > 0).all(), what
    first = [int(np.flatnonzero(classes == c)[0]) for c in range(len(reps))]
    assert first == reps.tolist() and int(sizes.sum()) == len(classes), what
    assert ((quot[:, np.arange(len(reps)), np.arange(len(reps))] == cc.NONE).all(axis=0) | (sizes > 1)).all(), what
    assert (expand_classes(classes, self_, quot) == m).all(), what + ": expand_classes"
    assert (cc.expand(classes, self_, quot) == m).all(), what


@pytest.mark.parametrize("name", cc.NAMES)
def test_host_equals_the_definition_on_synthetic_matrices(name):
    m = cc.synthetic(name)
    h = Host(m)
    assert h.call() == 0
    check(h.result(), cc.synthetic_ref(name), m, name)
    assert int(h.out["rounds"][0]) == 1
    assert (h.out["verdict_out"] == m).all()
    if name.startswith("planted_"):
        n, p, c = (int(x) for x in name.split("_")[1:])
        assert m.shape == (p, n, n) and int(h.out["n_classes"][0]) <= c


def test_the_small_cases_by_hand():
    want = {"planted_1_1_1": [0], "planted_2_1_1": [0, 0], "asym_pair": [0, 0, 1, 0, 2, 0], "diag_pair": [0, 0, 0, 1, 0]}
    for name, classes in want.items():
        assert cc.synthetic_ref(name)[0].tolist() == classes, name
    assert len(cc.synthetic_ref("equal")[1]) == 1 and len(cc.synthetic_ref("random")[1]) == 130
    assert len(cc.synthetic_ref("planted_64_1_64")[1]) > 32
    assert set(np.unique(cc.synthetic("bytes")).tolist()) >= {0xA5, 255}
    s = cc.synthetic("symmetric")
    assert (s == s.transpose(0, 2, 1)).all() and set(np.unique(s).tolist()) == {0, 1}
    c1, _, _, self_, quot = cc.synthetic_ref("diag_pair")
    assert self_.tolist() == [[1, 0]] and quot.tolist() == [[[1, 1], [1, 255]]]


@pytest.mark.parametrize("fam, n_classes", [(4, 18), (16, 27)])
def test_host_equals_the_definition_on_the_oracle_matrices(fam, n_classes):
    m = rc.case(fam)["want"]
    want = cc.oracle_ref(fam)
    C_ = len(want[1])
    assert 1 < C_ < rc.N_EP and C_ == n_classes
    if fam == 4:
        assert want[2].tolist() == [2, 5, 2, 1, 5, 3, 2, 1, 2, 1, 1, 1, 1, 4, 2, 1, 1, 2]
    else:
        # one class of 5, six of 2 and 20 of 1: 27 classes over 37 endpoints
        assert sorted(want[2].tolist(), reverse=True)[:8] == [5] + [2] * 6 + [1]
    h = Host(m)
    assert h.call() == 0 and int(h.out["n_classes"][0]) == C_ and int(h.out["rounds"][0]) == 1
    check(h.result(), want, m, "family %d" % fam)


def test_class_cap_too_small_leaves_the_per_class_outputs():
    m = cc.synthetic("planted_65_2_7")
    want = cc.synthetic_ref("planted_65_2_7")
    c = len(want[1])
    h = Host(m, cap=c - 1)
    assert h.call() == 0
    assert int(h.out["n_classes"][0]) == c and (h.out["class_out"] == want[0]).all()
    assert h.untouched("rep_out", "size_out", "self_out", "quot_out")
    h = Host(m, cap=c)                                   # room for exactly C
    assert h.call() == 0
    check(h.result(), want, m, "cap == C")
    # output subsets: the count alone; the classes alone
    h = Host(m)
    none = dict.fromkeys(("class_out", "rep_out", "size_out", "self_out", "quot_out", "verdict_out", "rounds",
                          "sums_out"))
    assert h.call(cap=0, **none) == 0 and int(h.out["n_classes"][0]) == c and h.untouched("class_out", "rep_out")
    h.fill()
    assert h.call(cap=0, **dict(none, n_classes=None, class_out=h.out["class_out"].ctypes.data)) == 0
    assert (h.out["class_out"] == want[0]).all() and h.untouched("n_classes", "rounds", "sums_out")


# the cases that take more than one round, by key width (from running them: the
# seeds are constants, so the counts are the same everywhere); every other one
# takes one
ROUNDS = {
    3: {"planted_63_3_5": 2, "planted_64_1_64": 2, "planted_65_2_7": 2, "planted_1000_2_40": 3,
        "planted_64_1_40": 2, "symmetric": 2, "random": 3},
    4: {"planted_64_1_64": 2, "planted_1000_2_40": 2, "planted_64_1_40": 2, "symmetric": 2, "random": 2},
    6: {"planted_64_1_64": 2, "planted_1000_2_40": 2, "random": 2},
    8: {},
}


@pytest.mark.parametrize("bits", [3, 4, 6, 8])
def test_truncated_keys_give_the_same_classes(bits):
    """key_bits forces collisions: candidates too coarse, caught by the verify
    pass and refined by further rounds; the classes are those of the full
    width, and the sums are the full-width round's when one round is enough."""
    for name in cc.NAMES:
        m = cc.synthetic(name)
        h = Host(m)
        assert h.call(key_bits=bits) == 0, (name, bits)
        check(h.result(), cc.synthetic_ref(name), m, "%s at %d bits" % (name, bits))
        rounds = int(h.out["rounds"][0])
        assert rounds == ROUNDS[bits].get(name, 1), (name, bits, rounds)
        if rounds == 1:
            full = Host(m)
            assert full.call() == 0 and (full.out["sums_out"] == h.out["sums_out"]).all()


def test_no_key_bits_do_not_converge():
    """key_bits = 0 leaves the diagonal alone in the keys: two classes with
    equal diagonals stay together in every round: CLS_E_INVAL, outputs alone.
    A matrix whose classes differ on the diagonal still converges."""
    h = Host(cc.synthetic("asym_pair"))
    assert h.call(key_bits=0) == _abi.E_INVAL and h.untouched()
    h = Host(cc.synthetic("diag_pair"))
    assert h.call(key_bits=0) == 0 and h.out["class_out"].tolist() == [0, 0, 0, 1, 0]
    h = Host(cc.synthetic("equal"))
    assert h.call(key_bits=0) == 0 and int(h.out["n_classes"][0]) == 1


def test_refusals_leave_the_outputs_alone():
    h = Host(cc.synthetic("planted_3_1_2"))
    refused = {
        "matrix NULL": lambda: h.call(matrix=False),
        "N = 0": lambda: h.call(N=0),
        "P = 0": lambda: h.call(P=0),
        "out NULL": lambda: h.call(out=False),
        "key_bits 65": lambda: h.call(key_bits=65),
        "N > 32768": lambda: h.call(N=32769),
        "P N^2 > 2^36": lambda: h.call(N=32768, P=65),
        "neither class_out nor n_classes": lambda: h.call(class_out=None, n_classes=None),
        "per-class outputs with class_cap 0": lambda: h.call(cap=0),
        "quot_out alone with class_cap 0": lambda: h.call(cap=0, rep_out=None, size_out=None, self_out=None),
    }
    for what, f in refused.items():
        h.fill()
        assert f() == _abi.E_INVAL, what
        assert h.untouched(), what
    assert h.call() == 0
    check(h.result(), cc.synthetic_ref("planted_3_1_2"), h.m, "after the refusals")


def test_null_arguments_are_refused():
    """cls_reach_classes with a NULL engine: CLS_E_INVAL, nothing written
    (with an engine: tests/test_gpu_reach_classes.py)."""
    fn = _abi.lib().cls_reach_classes
    h = Host(cc.synthetic("planted_3_1_2"))
    spec = _abi.ReachSpec(_abi.AF_V4, 3, None, None, None, 1, None, None, None)
    o = {k: v.ctypes.data for k, v in h.out.items()}
    o["class_cap"] = 3
    st = _abi.ReachClassesOut(*[o[k] for k in FIELDS])
    for s, oo in ((C.byref(spec), C.byref(st)), (None, C.byref(st)), (C.byref(spec), None), (None, None)):
        for mat in (h.m.ctypes.data, None):
            for flags in (0, _abi.F_DEVICE):
                assert fn(None, s, mat, oo, flags, None) == _abi.E_INVAL
    assert h.untouched()


def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "contivcls.h")).read()
    for sym in ("cls_reach_classes", "cls_reach_classes_host"):
        assert sym in _abi.SYMBOLS and hasattr(_abi.lib(), sym)
        assert re.search(r"^int %s\(" % sym, hdr, re.M)
    assert re.search(r"^#define CLS_CLASS_NONE 255u\b", hdr, re.M) and _abi.CLASS_NONE == 255
    assert re.search(r"^#define CLS_ABI_VERSION 5$", hdr, re.M) and _abi.lib().cls_abi_version() == 5
    assert "classes_key_bits" in hdr and "RETURNS ONLY WHEN THE RESULT IS" in hdr


def test_layout_matches_the_header():
    """cls_reach_classes_out as the C compiler lays it out (LP64)."""
    assert [f for f, _ in _abi.ReachClassesOut._fields_] == FIELDS
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "contivcls.h"\nint main(void) {\n'
           'printf("%zu", sizeof(cls_reach_classes_out));\n' +
           "".join('printf(" %%zu", offsetof(cls_reach_classes_out, %s));\n' % f for f in FIELDS) +
           'printf(" %u", CLS_CLASS_NONE);\nreturn 0; }\n')
    exe = os.path.join(ROOT, "go", "shimtest", "reach_classes_layout_cpu_check")
    try:
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-x", "c",
                            "-", "-o", exe], input=src, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    finally:
        if os.path.exists(exe):
            os.remove(exe)
    assert got[0] == C.sizeof(_abi.ReachClassesOut)
    assert got[1:-1] == [getattr(_abi.ReachClassesOut, f).offset for f in FIELDS]
    assert got[-1] == 255


def test_classes_key_bits_option_is_checked():
    """classes_key_bits through the options reader (cls_compile_v4's option
    string takes every key of cls_engine_set_option): 0 .. 64."""
    from aclgen import random_acl
    rules, _ = random_acl(1, 12, 0.0)
    cr = _abi.CRules(rules)
    need = C.c_uint64(0)
    f = _abi.lib().cls_compile_v4
    for ok in (b"classes_key_bits=0", b"classes_key_bits=4", b"classes_key_bits=64", b"reach_tile=1024,classes_key_bits=8"):
        assert f(cr.ptr(), cr.n, None, 0, C.byref(need), ok) == 0, ok
    for bad in (b"classes_key_bits=65", b"classes_key_bits=-1", b"classes_key_bits=", b"classes_key_bits"):
        assert f(cr.ptr(), cr.n, None, 0, C.byref(need), bad) == _abi.E_INVAL, bad


def test_classes_shims_compile_as_c99():
    """contivcls_go.h with the classes shims, and go/shimtest/reachclasses.c
    that calls them, as strict C99 (gcc -std=c99 -Werror), linked to the
    library."""
    hdr = open(os.path.join(ROOT, "include", "contivcls_go.h")).read()
    assert "clsg_reach_classes_v4(" in hdr and "clsg_reach_classes_v16(" in hdr
    out = os.path.join(ROOT, "go", "shimtest", "reachclasses_cpu_check")
    try:
        r = subprocess.run(["gcc", "-O1", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                            "-I" + os.path.join(ROOT, "include"), "-o", out,
                            os.path.join(ROOT, "go", "shimtest", "reachclasses.c"),
                            "-L" + os.path.join(ROOT, "vpp_amd"), "-lcontivcls",
                            "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    finally:
        if os.path.exists(out):
            os.remove(out)
    mk = open(os.path.join(ROOT, "go", "shimtest", "Makefile")).read()
    assert re.search(r"^all:.*\$\(HERE\)reachclasses\b", mk, re.M) and re.search(r"rm -f .*\$\(HERE\)reachclasses\b", mk)


def test_go_binding_calls_the_classes_shims_with_go19_api():
    from test_go_binding_cpu import POST_19, _code
    code = _code(GO)
    assert "C.clsg_reach_classes_v4(" in code and "C.clsg_reach_classes_v16(" in code
    # only through the shims: neither the entry point nor its structure
    assert "C.cls_reach_classes" not in code
    for pat in POST_19:
        assert not re.search(pat, code), pat
