"""CPU checks of the hop closure's boundary (cls_reach_hops): the entry point
refuses a null engine, spec or out without touching a device or an output,
cls_reach_hops_out is laid out as the header's, the symbol is declared and
exported, the hops_rows option is read by the options reader, the tests'
numpy definition (reach_hops_cases.hops_ref) agrees with an independent
per-source queue search on the synthetic graphs and on hand-made ones, the
oracle case the GPU tests use is not degenerate, the Go shims and
go/shimtest/reachhops.c compile as strict C99, and the Go binding calls only
the shims with Go 1.9 API."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reach_cases as rc
import reach_hops_cases as hc
from vpp_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "go", "contivcls", "contivcls.go")


def test_null_arguments_are_refused():
    """A NULL engine with and without a NULL spec, matrix or out:
    CLS_E_INVAL, nothing written (with an engine: tests/test_gpu_reach_hops.py)."""
    fn = _abi.lib().cls_reach_hops
    n = 3
    spec = _abi.ReachSpec(_abi.AF_V4, n, None, None, None, 1, None, None, None)
    m = np.full((1, n, n), 2, np.uint8)
    outs = [np.full((n, n), 9, np.uint8), np.full(n, 9, np.uint32), np.full(n, 9, np.uint32),
            np.full(256, 9, np.uint64), np.full((n, 1), 9, np.uint64)]
    o = _abi.ReachHopsOut(*[x.ctypes.data for x in outs])
    for s, oo in ((C.byref(spec), C.byref(o)), (None, C.byref(o)), (C.byref(spec), None), (None, None)):
        for mat in (m.ctypes.data, None):
            for flags in (0, _abi.F_DEVICE):
                assert fn(None, s, mat, 0, oo, flags, None) == _abi.E_INVAL
    for x in outs:
        assert x.tobytes() == np.full(x.shape, 9, x.dtype).tobytes()


def test_symbol_is_declared_and_exported():
    assert "cls_reach_hops" in _abi.SYMBOLS
    assert hasattr(_abi.lib(), "cls_reach_hops")
    hdr = open(os.path.join(ROOT, "include", "contivcls.h")).read()
    assert re.search(r"^int cls_reach_hops\(", hdr, re.M)
    assert re.search(r"^#define CLS_HOPS_NONE 255u\b", hdr, re.M) and _abi.HOPS_NONE == 255
    assert re.search(r"^#define CLS_ABI_VERSION 5$", hdr, re.M) and _abi.lib().cls_abi_version() == 5


def test_layout_matches_the_header():
    """cls_reach_hops_out as the C compiler lays it out (LP64): the ctypes
    structure's size and field offsets, in the header's order."""
    names = [f for f, _ in _abi.ReachHopsOut._fields_]
    assert names == ["hops_out", "reach_out", "exposed_out", "level_out", "closure_out"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "contivcls.h"\nint main(void) {\n'
           'printf("%zu", sizeof(cls_reach_hops_out));\n' +
           "".join('printf(" %%zu", offsetof(cls_reach_hops_out, %s));\n' % f for f in names) +
           'printf(" %u", CLS_HOPS_NONE);\nreturn 0; }\n')
    exe = os.path.join(ROOT, "go", "shimtest", "reach_hops_layout_cpu_check")
    try:
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-x", "c",
                            "-", "-o", exe], input=src, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    finally:
        if os.path.exists(exe):
            os.remove(exe)
    assert got[0] == C.sizeof(_abi.ReachHopsOut)
    assert got[1:-1] == [getattr(_abi.ReachHopsOut, f).offset for f in names]
    assert got[-1] == 255


def test_hops_rows_option_is_checked():
    """hops_rows through the options reader (cls_compile_v4's option string
    takes every key of cls_engine_set_option): 0, 4, 8 or 16."""
    from aclgen import random_acl
    rules, _ = random_acl(1, 12, 0.0)
    cr = _abi.CRules(rules)
    need = C.c_uint64(0)
    f = _abi.lib().cls_compile_v4
    for ok in (b"hops_rows=0", b"hops_rows=4", b"hops_rows=8", b"hops_rows=16", b"reach_tile=1024,hops_rows=4"):
        assert f(cr.ptr(), cr.n, None, 0, C.byref(need), ok) == 0, ok
    for bad in (b"hops_rows=1", b"hops_rows=5", b"hops_rows=32", b"hops_rows=-8", b"hops_rows=", b"hops_rows"):
        assert f(cr.ptr(), cr.n, None, 0, C.byref(need), bad) == _abi.E_INVAL, bad


def _queue_bfs(adj, H):
    """Per source, a first-in first-out search over adjacency lists."""
    n = len(adj)
    out = np.full((n, n), 255, np.uint8)
    nbr = [[d for d in range(n) if adj[s][d] and d != s] for s in range(n)]
    for s in range(n):
        dist = {s: 0}
        q = collections.deque([s])
        while q:
            u = q.popleft()
            if dist[u] == H:
                continue
            for v in nbr[u]:
                if v not in dist:
                    dist[v] = dist[u] + 1
                    q.append(v)
        for d, k in dist.items():
            out[s, d] = k
    return out


@pytest.mark.parametrize("name", hc.GRAPHS)
def test_hops_ref_equals_a_queue_search(name):
    for n in (1, 2, 5, 64, 65, 129):
        m, a = hc.synthetic(name, n, 3)
        assert (hc.adjacency(m) & ~np.eye(n, dtype=bool) == a).all()
        assert set(np.unique(m).tolist()) <= {0, 1, 2, 3} and (m[:, np.arange(n), np.arange(n)] == 2).all()
        for H in (0, 1, 3):
            want = _queue_bfs(a.tolist(), H or 254)
            # (ALLOW on the diagonal is ignored)
            got = hc.hops_ref(hc.adjacency(m), H)
            assert (got == want).all(), (name, n, H)
    assert (hc.synthetic_ref(name, 65)[0] == hc.hops_ref(hc.graph(name, 65))).all()


def test_hops_ref_and_sums_on_hand_made_graphs():
    # 0 -> 1 -> 2, 3 alone, 2 -> 0
    a = np.zeros((4, 4), bool)
    a[0, 1] = a[1, 2] = a[2, 0] = True
    h = hc.hops_ref(a)
    assert h.tolist() == [[0, 1, 2, 255], [2, 0, 1, 255], [1, 2, 0, 255], [255, 255, 255, 0]]
    assert hc.hops_ref(a, 1).tolist() == [[0, 1, 255, 255], [255, 0, 1, 255], [1, 255, 0, 255], [255, 255, 255, 0]]
    reach, exposed, levels, closure = hc.sums(h)
    assert reach.tolist() == [2, 2, 2, 0] and exposed.tolist() == [2, 2, 2, 0]
    assert levels[[0, 1, 2, 255]].tolist() == [4, 3, 3, 6] and levels.sum() == 16 and len(levels) == 256
    assert closure.shape == (4, 1) and closure[:, 0].tolist() == [0b0111, 0b0111, 0b0111, 0b1000]
    # a path of 300: 254 hops are counted, the 255th is out of reach; the
    # closure has five words with zero padding
    p = hc.hops_ref(hc.graph("path", 300))
    assert p[0, 254] == 254 and p[0, 255] == 255 and p[45, 299] == 254 and p[44, 299] == 255 and p[1, 0] == 255
    _, _, lv, cl = hc.sums(p)
    assert cl.shape == (300, 5) and int(cl[0, 3]) == (1 << 63) - 1 and int(cl[0, 4]) == 0
    assert int(cl[299, 4]) == 1 << (299 - 256) and lv[1] == 299 and lv[254] == 46
    assert lv[255] == 300 * 300 - 300 - sum(300 - k for k in range(1, 255))


@pytest.mark.parametrize("fam, at1, at2, none", [(4, 364, 36, 932), (16, 444, 62, 826)])
def test_the_oracle_case_is_not_degenerate(fam, at1, at2, none):
    """The 37 endpoints x 3 probes of reach_cases on the oracle alone: pairs
    at 1, 2 and no hops, and probe 0 of the IPv4 case alone differs."""
    want = rc.case(fam)["want"]
    lv = hc.sums(hc.hops_ref(hc.adjacency(want)))[2]
    assert lv[[0, 1, 2, 255]].tolist() == [37, at1, at2, none] and lv.sum() == 37 * 37
    if fam == 4:
        one = hc.sums(hc.hops_ref(hc.adjacency(want[:1])))[2]
        assert one[[0, 1, 2, 255]].tolist() == [37, 104, 52, 1176]


def test_hops_shims_compile_as_c99():
    """contivcls_go.h with the hop-closure shims, and go/shimtest/reachhops.c
    that calls them, as strict C99 (gcc -std=c99 -Werror), linked to the
    library."""
    hdr = open(os.path.join(ROOT, "include", "contivcls_go.h")).read()
    assert "clsg_reach_hops_v4(" in hdr and "clsg_reach_hops_v16(" in hdr
    out = os.path.join(ROOT, "go", "shimtest", "reachhops_cpu_check")
    try:
        r = subprocess.run(["gcc", "-O1", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                            "-I" + os.path.join(ROOT, "include"), "-o", out,
                            os.path.join(ROOT, "go", "shimtest", "reachhops.c"),
                            "-L" + os.path.join(ROOT, "vpp_amd"), "-lcontivcls",
                            "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    finally:
        if os.path.exists(out):
            os.remove(out)
    mk = open(os.path.join(ROOT, "go", "shimtest", "Makefile")).read()
    assert re.search(r"^all:.*\$\(HERE\)reachhops\b", mk, re.M) and re.search(r"rm -f .*\$\(HERE\)reachhops\b", mk)


def test_go_binding_calls_the_hops_shims_with_go19_api():
    from test_go_binding_cpu import POST_19, _code
    code = _code(GO)
    assert "C.clsg_reach_hops_v4(" in code and "C.clsg_reach_hops_v16(" in code
    # only through the shims: neither the entry point nor its structure
    assert "C.cls_reach_hops" not in code
    for pat in POST_19:
        assert not re.search(pat, code), pat
