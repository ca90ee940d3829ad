"""CPU checks of the port sweep's boundary (cls_reach_ports,
cls_port_classes): the entry point refuses null arguments without touching a
device, the record and the output structure are laid out as the header's,
cls_port_classes returns class starts inside which no rule's port range
begins or ends, the tests' numpy definition (reach_ports_cases.ranges_ref) is
right on hand-made arrays, the case the GPU tests sweep is not degenerate and
its brute force over all 65,536 ports changes verdict only on class starts,
the Go shims and go/shimtest/reachports.c compile as strict C99, and the Go
binding calls only the shims with Go 1.9 API."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reach_cases as rc
import reach_ports_cases as pc
from vpp_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "go", "contivcls", "contivcls.go")


def test_null_arguments_are_refused():
    """A NULL engine with and without a NULL spec or out: CLS_E_INVAL, nothing
    written (with an engine: tests/test_gpu_reach_ports.py)."""
    fn = _abi.lib().cls_reach_ports
    assert "cls_reach_ports" in _abi.SYMBOLS and "cls_port_classes" in _abi.SYMBOLS
    n = 3
    keep = [np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(1, np.uint8), np.zeros(1, np.uint16)]
    spec = _abi.ReachSpec(_abi.AF_V4, n, keep[0].ctypes.data, keep[1].ctypes.data, None, 1, keep[2].ctypes.data,
                          keep[3].ctypes.data, None)
    outs = [np.full(18, 9, _abi.PORT_RANGE), np.full(1, 9, np.uint64), np.full(9, 9, np.uint32),
            np.full(9, 9, np.uint32), np.full(4, 9, np.uint64), np.full(1, 9, np.uint32)]
    rg, nr, ru, al, hi, k = (x.ctypes.data for x in outs)
    o = _abi.ReachPortsOut(rg, 18, nr, ru, al, hi, k)
    for s, oo in ((C.byref(spec), C.byref(o)), (None, C.byref(o)), (C.byref(spec), None), (None, None)):
        for flags in (0, _abi.F_DEVICE):
            assert fn(None, s, oo, flags, None) == _abi.E_INVAL
    for x in outs:
        assert x.tobytes() == np.full(x.shape, 9, x.dtype).tobytes()
    # cls_port_classes: n is required, rules too when there are any
    lo, cnt = np.full(4, 9, np.uint16), C.c_uint32(9)
    assert _abi.lib().cls_port_classes(None, 0, 0, lo.ctypes.data, 4, None) == _abi.E_INVAL
    assert _abi.lib().cls_port_classes(None, 2, 0, lo.ctypes.data, 4, C.byref(cnt)) == _abi.E_INVAL
    assert (lo == 9).all() and cnt.value == 9
    assert _abi.lib().cls_port_classes(None, 0, 0, lo.ctypes.data, 4, C.byref(cnt)) == 0
    assert cnt.value == 1 and lo.tolist() == [0, 9, 9, 9]


def _layout(struct, fields):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "contivcls.h"\nint main(void) {\n'
           'printf("%%zu", sizeof(%s));\n' % struct +
           "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) + "return 0; }\n")
    exe = os.path.join(ROOT, "go", "shimtest", "reach_ports_layout_cpu_check")
    try:
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-x", "c",
                            "-", "-o", exe], input=src, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    finally:
        if os.path.exists(exe):
            os.remove(exe)


@pytest.mark.parametrize("struct, ct", [("cls_port_range", _abi.PortRange),
                                        ("cls_reach_ports_out", _abi.ReachPortsOut)])
def test_layouts_match_the_header(struct, ct):
    """Both structures as the C compiler lays them out (LP64): the ctypes
    structures' sizes and field offsets; the record is 16 bytes and the numpy
    dtype is the same record."""
    names = [f for f, _ in ct._fields_]
    got = _layout(struct, names)
    assert got[0] == C.sizeof(ct)
    assert got[1:] == [getattr(ct, f).offset for f in names]
    if ct is _abi.PortRange:
        assert got[0] == 16 and _abi.PORT_RANGE.itemsize == 16
        assert [_abi.PORT_RANGE.fields[f][1] for f in names] == got[1:]
        assert names == ["src", "dst", "port_lo", "port_hi", "action", "zero"]


def _acls():
    from aclgen import many_ports_acl, random_acl, random_acl16, single_port_acl
    out = []
    for weird in (0.0, 0.003, 0.15):
        out.append(("random_acl %g" % weird, random_acl(31, 300, weird=weird)[0]))
        out.append(("random_acl16 %g" % weird, random_acl16(32, 300, weird=weird)[0]))
    many, single = many_ports_acl(5), single_port_acl(6)
    out.append(("many_ports_acl", many[0] if isinstance(many, tuple) else many))
    out.append(("single_port_acl", single[0] if isinstance(single, tuple) else single))
    return out


@pytest.mark.parametrize("proto", [0, 1, 2, 47])
def test_port_classes_of_random_acls(proto):
    """cls_port_classes on random ACLs with malformed rules (reversed ranges,
    70000-80000, 65536 + 80), many distinct ranges and single ports: the
    starts ascend from 0, each is 0, a rule's lo16 or hi16 + 1, and over all
    65,536 ports the set of rules whose [lo16, hi16] holds the port is
    constant inside a class; ICMP and protocol 47 have one class; a cap too
    small sets only the count."""
    from vpp_amd.engine import Engine
    ports = np.arange(65536)
    widest = 0
    for what, rules in _acls():
        lo = Engine.port_classes(rules, proto)
        assert lo.dtype == np.uint16 and lo[0] == 0 and (np.diff(lo.astype(np.int64)) > 0).all(), what
        ok, pairs = pc.allowed_starts(rules, proto)
        assert set(lo.tolist()) <= ok, (what, sorted(set(lo.tolist()) - ok)[:8])
        if proto > 1:
            assert len(lo) == 1 and not pairs, what
            continue
        widest = max(widest, len(lo))
        # the class of every port; a rule's range must hold whole classes
        cls = np.searchsorted(lo, ports, side="right") - 1
        for a, b in set(pairs):
            inside = (ports >= a) & (ports <= b)
            per = np.bincount(cls, inside, len(lo))
            assert ((per == 0) | (per == np.bincount(cls, minlength=len(lo)))).all(), (what, a, b)
        assert (pc.class_starts([rules], proto) == lo).all(), what
        # cap one short: only the count
        cr = _abi.CRules(rules)
        buf, cnt = np.full(len(lo), 0xA5A5, np.uint16), C.c_uint32(0)
        assert _abi.lib().cls_port_classes(cr.ptr(), cr.n, proto, buf.ctypes.data, len(lo) - 1, C.byref(cnt)) == 0
        assert cnt.value == len(lo) and (buf == 0xA5A5).all(), what
        assert _abi.lib().cls_port_classes(cr.ptr(), cr.n, proto, buf.ctypes.data, len(lo), C.byref(cnt)) == 0
        assert (buf == lo).all(), what
    assert proto > 1 or widest > 256


def _rows(rec):
    return [(int(r["src"]), int(r["dst"]), int(r["port_lo"]), int(r["port_hi"]), int(r["action"])) for r in rec]


def test_ranges_ref_on_hand_made_arrays():
    v = np.zeros((2, 2, 65536), np.uint8)
    v[0, 0] = 2                                        # a single range
    v[0, 1, 1:] = 2                                    # a change at 0 -> 1
    v[1, 0, 65535] = 3                                 # a change at 65534 -> 65535
    v[1, 1, 100:200], v[1, 1, 200:300] = 2, 1
    rec, total, runs, allow, hist = pc.ranges_ref(v)
    assert total == 9 and rec.dtype == _abi.PORT_RANGE and not rec["zero"].any()
    assert _rows(rec) == [(0, 0, 0, 65535, 2), (0, 1, 0, 0, 0), (0, 1, 1, 65535, 2), (1, 0, 0, 65534, 0),
                          (1, 0, 65535, 65535, 3), (1, 1, 0, 99, 0), (1, 1, 100, 199, 2), (1, 1, 200, 299, 1),
                          (1, 1, 300, 65535, 0)]
    assert runs.tolist() == [[1, 2], [2, 4]] and runs.dtype == np.uint32
    assert allow.tolist() == [[65536, 65535], [0, 100]] and allow.dtype == np.uint32
    assert hist.tolist() == [1 + 65535 + 65536 - 200, 100, 65536 + 65535 + 100, 1] and hist.sum() == 4 * 65536
    # the same verdicts at class starts: equal neighbours across a class
    # boundary merge, whatever the decomposition
    for starts in ([0, 1, 100, 200, 300, 65535], [0, 1, 2, 50, 100, 150, 200, 250, 300, 4000, 65534, 65535]):
        got = pc.ranges_ref(v[:, :, starts], starts)
        assert got[1] == total and got[0].tobytes() == rec.tobytes()
        assert (got[2] == runs).all() and (got[3] == allow).all() and (got[4] == hist).all()
    # cap cuts the records, not the total
    rec3, total3, _, _, _ = pc.ranges_ref(v, cap=3)
    assert total3 == 9 and rec3.tobytes() == rec[:3].tobytes()


@pytest.mark.parametrize("proto", [0, 1])
@pytest.mark.parametrize("fam", [4, 16])
def test_the_case_is_not_degenerate(fam, proto):
    """The six endpoints the GPU tests sweep, on the oracle alone: many pairs
    with several ranges, every ConnectionAction, enough classes -- and every
    change of verdict of the brute force over all ports on a class start of
    the restatement, which is what makes one representative per class exact."""
    eps, v = pc.brute(fam, proto)
    assert v.shape == (6, 6, 65536) and len(set(eps.tolist())) == 6
    _, total, runs, allow, hist = pc.ranges_ref(v)
    assert (runs > 1).sum() >= 8 and runs.max() >= 3 and total == runs.sum()
    assert set(np.unique(v).tolist()) == {0, 1, 2, 3}
    assert hist.sum() == 36 * 65536 and (allow <= 65536).all()
    starts = pc.class_starts(pc.bound_rules(rc.case(fam), eps), proto)
    assert len(starts) >= 65
    changes = np.unique(np.argwhere(v[:, :, 1:] != v[:, :, :-1])[:, 2] + 1)
    assert len(changes) >= 3 and np.isin(changes, starts).all()
    # hence the verdicts at the class starts alone give the same ranges
    at = pc.ranges_ref(v[:, :, starts], starts)
    assert at[1] == total and at[0].tobytes() == pc.ranges_ref(v)[0].tobytes()


@pytest.mark.parametrize("fam", [4, 16])
def test_all_endpoints_have_many_classes(fam):
    """All 37 endpoints bind enough ACLs for more than 256 classes, so a
    pair's rows outgrow a wave."""
    c = rc.case(fam)
    for proto in (0, 1):
        assert len(pc.class_starts(pc.bound_rules(c, np.arange(rc.N_EP)), proto)) >= 257


def test_ports_shims_compile_as_c99():
    """contivcls_go.h with the port-sweep shims, and go/shimtest/reachports.c
    that calls them, as strict C99 (gcc -std=c99 -Werror), linked to the
    library."""
    hdr = open(os.path.join(ROOT, "include", "contivcls_go.h")).read()
    assert "clsg_reach_ports_v4(" in hdr and "clsg_reach_ports_v16(" in hdr
    out = os.path.join(ROOT, "go", "shimtest", "reachports_cpu_check")
    try:
        r = subprocess.run(["gcc", "-O1", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                            "-I" + os.path.join(ROOT, "include"), "-o", out,
                            os.path.join(ROOT, "go", "shimtest", "reachports.c"),
                            "-L" + os.path.join(ROOT, "vpp_amd"), "-lcontivcls",
                            "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    finally:
        if os.path.exists(out):
            os.remove(out)
    mk = open(os.path.join(ROOT, "go", "shimtest", "Makefile")).read()
    assert re.search(r"^all:.*\$\(HERE\)reachports\b", mk, re.M) and re.search(r"rm -f .*\$\(HERE\)reachports\b", mk)


def test_go_binding_calls_the_ports_shims_with_go19_api():
    from test_go_binding_cpu import POST_19, _code
    code = _code(GO)
    assert "C.clsg_reach_ports_v4(" in code and "C.clsg_reach_ports_v16(" in code
    # only through the shims: neither the entry point nor its structures
    assert "C.cls_reach_ports" not in code and "C.cls_port_range" not in code
    for pat in POST_19:
        assert not re.search(pat, code), pat
