"""CPU checks of the reachability matrix's boundary (cls_reach_matrix): the
entry point refuses a null engine or spec without touching a device, the
reach_tile option is read by the options reader, the Go shims compile as
strict C99 and the Go binding calls them with Go 1.9 API only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from vpp_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "go", "contivcls", "contivcls.go")


def _spec(n=3, p=2):
    keep = [np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(p, np.uint8), np.zeros(p, np.uint16),
            np.zeros(p, np.uint16)]
    s = _abi.ReachSpec(_abi.AF_V4, n, keep[0].ctypes.data, keep[1].ctypes.data, None, p, keep[2].ctypes.data,
                       keep[3].ctypes.data, keep[4].ctypes.data)
    return s, keep


def test_null_engine_and_null_spec_are_refused():
    fn = _abi.lib().cls_reach_matrix
    assert "cls_reach_matrix" in _abi.SYMBOLS
    s, keep = _spec()
    v, h, a = np.full(18, 9, np.uint8), np.full(8, 9, np.uint64), np.full(6, 9, np.uint32)
    assert fn(None, C.byref(s), v.ctypes.data, h.ctypes.data, a.ctypes.data, 0, None) == _abi.E_INVAL
    assert fn(None, None, v.ctypes.data, h.ctypes.data, a.ctypes.data, 0, None) == _abi.E_INVAL
    assert fn(None, None, None, None, None, _abi.F_DEVICE | _abi.F_NO_VERDICT, None) == _abi.E_INVAL
    assert (v == 9).all() and (h == 9).all() and (a == 9).all()


def test_reach_spec_layout_matches_the_header():
    """cls_reach_spec as the C compiler lays it out (LP64): the ctypes
    structure's size and field offsets."""
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "contivcls.h"\nint main(void) {\n'
           'printf("%zu", sizeof(cls_reach_spec));\n' +
           "".join('printf(" %%zu", offsetof(cls_reach_spec, %s));\n' % f for f, _ in _abi.ReachSpec._fields_) +
           "return 0; }\n")
    exe = os.path.join(ROOT, "go", "shimtest", "reach_layout_cpu_check")
    try:
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-x", "c",
                            "-", "-o", exe], input=src, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    finally:
        if os.path.exists(exe):
            os.remove(exe)
    assert got[0] == C.sizeof(_abi.ReachSpec)
    assert got[1:] == [getattr(_abi.ReachSpec, f).offset for f, _ in _abi.ReachSpec._fields_]


def test_reach_tile_option_is_checked():
    """reach_tile through the options reader (cls_compile_v4's option string
    takes every key of cls_engine_set_option): 256 .. 2^30 connections."""
    from aclgen import random_acl
    rules, _ = random_acl(1, 12, 0.0)
    cr = _abi.CRules(rules)
    need = C.c_uint64(0)
    f = _abi.lib().cls_compile_v4
    for ok in (b"reach_tile=256", b"reach_tile=1024", b"reach_tile=1000", b"reach_tile=4194304",
               b"reach_tile=1073741824", b"orient=dst,reach_tile=0x100000"):
        assert f(cr.ptr(), cr.n, None, 0, C.byref(need), ok) == 0, ok
    for bad in (b"reach_tile=255", b"reach_tile=0", b"reach_tile=-1024", b"reach_tile=1073741825", b"reach_tile=1Mi",
                b"reach_tile=", b"reach_tile"):
        assert f(cr.ptr(), cr.n, None, 0, C.byref(need), bad) == _abi.E_INVAL, bad


def test_reach_shims_compile_as_c99():
    """contivcls_go.h with the reach shims, and go/shimtest/reachtest.c that
    calls them, as strict C99 (gcc -std=c99 -Werror), linked to the library."""
    hdr = open(os.path.join(ROOT, "include", "contivcls_go.h")).read()
    assert "clsg_reach_matrix_v4(" in hdr and "clsg_reach_matrix_v16(" in hdr
    out = os.path.join(ROOT, "go", "shimtest", "reachtest_cpu_check")
    try:
        r = subprocess.run(["gcc", "-O1", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                            "-I" + os.path.join(ROOT, "include"), "-o", out,
                            os.path.join(ROOT, "go", "shimtest", "reachtest.c"),
                            "-L" + os.path.join(ROOT, "vpp_amd"), "-lcontivcls",
                            "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    finally:
        if os.path.exists(out):
            os.remove(out)


def test_go_binding_calls_the_reach_shims_with_go19_api():
    from test_go_binding_cpu import POST_19, _code
    code = _code(GO)
    assert "C.clsg_reach_matrix_v4(" in code and "C.clsg_reach_matrix_v16(" in code
    assert "C.cls_reach_spec" not in code and "C.cls_reach_matrix(" not in code      # only through the shims
    for pat in POST_19:
        assert not re.search(pat, code), pat
