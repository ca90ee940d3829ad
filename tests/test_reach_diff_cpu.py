"""CPU checks of the reachability diff's boundary (cls_reach_diff): the entry
point refuses null arguments without touching a device, the record and the
output structure are laid out as the header's, the Go shims and
go/shimtest/reachdiff.c compile as strict C99, the Go binding calls only the
shims with Go 1.9 API, the tests' numpy definition (reach_diff_cases.diff_ref)
is right on hand-made matrices, and the ACL change the GPU tests use is not
degenerate."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reach_diff_cases as dc
from vpp_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "go", "contivcls", "contivcls.go")


def test_null_arguments_are_refused():
    """A NULL engine with and without a NULL spec, base or out: CLS_E_INVAL,
    nothing written (with an engine: tests/test_gpu_reach_diff.py)."""
    fn = _abi.lib().cls_reach_diff
    assert "cls_reach_diff" in _abi.SYMBOLS
    n, p = 3, 2
    keep = [np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(p, np.uint8), np.zeros(p, np.uint16),
            np.zeros(p, np.uint16)]
    spec = _abi.ReachSpec(_abi.AF_V4, n, keep[0].ctypes.data, keep[1].ctypes.data, None, p, keep[2].ctypes.data,
                          keep[3].ctypes.data, keep[4].ctypes.data)
    base = np.full(18, 9, np.uint8)
    outs = [np.full(18, 9, np.uint8), np.full(8, 9, np.uint64), np.full(6, 9, np.uint32),
            np.full(18, 9, _abi.REACH_CHANGE), np.full(1, 9, np.uint64), np.full(32, 9, np.uint64),
            np.full(6, 9, np.uint32)]
    v, h, a, ch, nc, tr, cd = (x.ctypes.data for x in outs)
    o = _abi.ReachDiffOut(v, h, a, ch, 18, nc, tr, cd)
    for s, b, oo in ((C.byref(spec), base.ctypes.data, C.byref(o)), (None, base.ctypes.data, C.byref(o)),
                     (C.byref(spec), None, C.byref(o)), (C.byref(spec), base.ctypes.data, None), (None, None, None)):
        for flags in (0, _abi.F_DEVICE):
            assert fn(None, s, b, oo, flags, None) == _abi.E_INVAL
    assert (base == 9).all()
    for x in outs:
        assert x.tobytes() == np.full(x.shape, 9, x.dtype).tobytes()


def _layout(struct, fields):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "contivcls.h"\nint main(void) {\n'
           'printf("%%zu", sizeof(%s));\n' % struct +
           "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) + "return 0; }\n")
    exe = os.path.join(ROOT, "go", "shimtest", "reach_diff_layout_cpu_check")
    try:
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-x", "c",
                            "-", "-o", exe], input=src, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    finally:
        if os.path.exists(exe):
            os.remove(exe)


@pytest.mark.parametrize("struct, ct", [("cls_reach_change", _abi.ReachChange),
                                        ("cls_reach_diff_out", _abi.ReachDiffOut)])
def test_layouts_match_the_header(struct, ct):
    """Both structures as the C compiler lays them out (LP64): the ctypes
    structures' sizes and field offsets; the record is 16 bytes and the numpy
    dtype is the same record."""
    names = [f for f, _ in ct._fields_]
    got = _layout(struct, names)
    assert got[0] == C.sizeof(ct)
    assert got[1:] == [getattr(ct, f).offset for f in names]
    if ct is _abi.ReachChange:
        assert got[0] == 16 and _abi.REACH_CHANGE.itemsize == 16
        assert [_abi.REACH_CHANGE.fields[f][1] for f in names] == got[1:]


def test_diff_shims_compile_as_c99():
    """contivcls_go.h with the diff shims, and go/shimtest/reachdiff.c that
    calls them, as strict C99 (gcc -std=c99 -Werror), linked to the library."""
    hdr = open(os.path.join(ROOT, "include", "contivcls_go.h")).read()
    assert "clsg_reach_diff_v4(" in hdr and "clsg_reach_diff_v16(" in hdr
    out = os.path.join(ROOT, "go", "shimtest", "reachdiff_cpu_check")
    try:
        r = subprocess.run(["gcc", "-O1", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                            "-I" + os.path.join(ROOT, "include"), "-o", out,
                            os.path.join(ROOT, "go", "shimtest", "reachdiff.c"),
                            "-L" + os.path.join(ROOT, "vpp_amd"), "-lcontivcls",
                            "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    finally:
        if os.path.exists(out):
            os.remove(out)
    mk = open(os.path.join(ROOT, "go", "shimtest", "Makefile")).read()
    assert re.search(r"^all:.*\$\(HERE\)reachdiff\b", mk, re.M) and re.search(r"rm -f .*\$\(HERE\)reachdiff\b", mk)


def test_go_binding_calls_the_diff_shims_with_go19_api():
    from test_go_binding_cpu import POST_19, _code
    code = _code(GO)
    assert "C.clsg_reach_diff_v4(" in code and "C.clsg_reach_diff_v16(" in code
    # only through the shims: neither the entry point nor its structures
    assert "C.cls_reach_diff" not in code and "C.cls_reach_change" not in code
    for pat in POST_19:
        assert not re.search(pat, code), pat


def test_diff_ref_on_hand_made_matrices():
    base = np.array([[[0, 1, 2], [3, 2, 2], [0, 0, 0]],
                     [[2, 2, 2], [2, 2, 2], [1, 1, 7]]], np.uint8)
    new = np.array([[[0, 1, 3], [3, 0, 2], [0, 0, 0]],
                    [[2, 2, 2], [0, 2, 2], [1, 1, 3]]], np.uint8)
    rec, total, trans, changed = dc.diff_ref(base, new)
    assert total == 4
    assert [tuple(int(x) for x in r) for r in rec] == [(0, 0, 2, 2, 3, 0), (0, 1, 1, 2, 0, 0), (1, 1, 0, 2, 0, 0),
                                                       (1, 2, 2, 7, 3, 0)]
    want = np.zeros((2, 4, 4), np.uint64)
    want[0, 0, 0], want[0, 1, 1], want[0, 2, 3], want[0, 3, 3], want[0, 2, 0], want[0, 2, 2] = 4, 1, 1, 1, 1, 1
    want[1, 2, 2], want[1, 2, 0], want[1, 1, 1], want[1, 3, 3] = 5, 1, 2, 1          # 7 & 3 = 3: on the diagonal
    assert (trans == want).all()
    assert changed.tolist() == [[1, 1, 0], [0, 1, 1]] and changed.dtype == np.uint32
    # cap cuts the records, not the total; nothing changed: empty
    rec2, total2, _, _ = dc.diff_ref(base, new, cap=3)
    assert total2 == 4 and rec2.tobytes() == rec[:3].tobytes()
    rec0, total0, trans0, changed0 = dc.diff_ref(new, new)
    assert total0 == 0 and len(rec0) == 0 and not changed0.any()
    assert all((trans0[p] == np.diag(np.diag(trans0[p]))).all() for p in range(2)) and trans0.sum() == 18


@pytest.mark.parametrize("fam", [4, 16])
def test_the_case_is_not_degenerate(fam):
    """The ACL change of the GPU tests, on the oracle's matrices alone: enough
    changed cells, in every probe, of several kinds, over many rows, and
    spread so that the cap values 100 and 200 end in tiles 0 and 1 of 1,024
    cells."""
    before, aft = dc.rc.case(fam)["want"], dc.after(fam)["want"]
    assert before.shape == aft.shape == (3, 37, 37) and before.size == 4107
    rec, total, trans, changed = dc.diff_ref(before, aft)
    cells = np.flatnonzero(before.ravel() != aft.ravel())
    assert 400 <= total <= 1000
    assert ((before != aft).reshape(3, -1).sum(axis=1) > 0).all()
    off = trans.sum(axis=0)
    off[np.arange(4), np.arange(4)] = 0
    assert (off > 0).sum() >= 5
    assert (changed > 0).sum() >= 60
    # cap 100 ends in tile 0 and cap 200 in tile 1: at least 100 but fewer
    # than 200 changed cells before cell 1,024, at least 200 before 2,048
    assert 100 <= (cells < 1024).sum() < 200
    assert (cells < 2048).sum() >= 200
    assert cells[99] < 1024 <= cells[199] < 2048
    # trans: row sums are the old histogram, column sums the new one
    for p in range(3):
        assert (trans[p].sum(axis=1) == np.bincount(before[p].ravel(), minlength=4)).all()
        assert (trans[p].sum(axis=0) == np.bincount(aft[p].ravel(), minlength=4)).all()
