"""CPU checks of the external sweep's boundary (cls_reach_external,
cls_addr_classes): the entry points refuse null arguments without touching a
device, the record and the output structure are laid out as the header's,
cls_addr_classes returns class starts on which the literal oracle's evalACL
is constant whatever the pod-side address and the position of the remote
address, the tests' numpy definition (reach_ext_cases.ranges_ref) is right on
hand-made arrays -- a single class of 2^32 addresses and a last class that
starts at 0xFFFFFFFF among them -- the case the GPU tests sweep is not
degenerate, the Go shims and go/shimtest/reachext.c compile as strict C99, and
the Go binding calls only the shims with Go 1.9 API."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import reach_cases as rc
import reach_ext_cases as xc
from vpp_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "go", "contivcls", "contivcls.go")


def test_null_arguments_are_refused():
    """A NULL engine with and without a NULL spec or out: CLS_E_INVAL, nothing
    written (with an engine: tests/test_gpu_reach_ext.py); cls_addr_classes
    needs n, and rules when there are any."""
    fn = _abi.lib().cls_reach_external
    assert "cls_reach_external" in _abi.SYMBOLS and "cls_addr_classes" in _abi.SYMBOLS
    n = 3
    keep = [np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(1, np.uint8), np.zeros(1, np.uint16),
            np.zeros(1, np.uint16)]
    spec = _abi.ReachSpec(_abi.AF_V4, n, keep[0].ctypes.data, keep[1].ctypes.data, None, 1, keep[2].ctypes.data,
                          keep[3].ctypes.data, keep[4].ctypes.data)
    outs = [np.full(18, 9, _abi.ADDR_RANGE), np.full(1, 9, np.uint64), np.full(6, 9, np.uint32),
            np.full(6, 9, np.uint64), np.full(8, 9, np.uint64), np.full(1, 9, np.uint32)]
    rg, nr, ru, al, hi, k = (x.ctypes.data for x in outs)
    o = _abi.ReachExtOut(rg, 18, nr, ru, al, hi, k)
    for s, oo in ((C.byref(spec), C.byref(o)), (None, C.byref(o)), (C.byref(spec), None), (None, None)):
        for flags in (0, _abi.F_DEVICE):
            assert fn(None, s, 0, 3, oo, flags, None) == _abi.E_INVAL
    for x in outs:
        assert x.tobytes() == np.full(x.shape, 9, x.dtype).tobytes()
    lo, cnt = np.full(4, 9, np.uint32), C.c_uint32(9)
    assert _abi.lib().cls_addr_classes(None, 0, lo.ctypes.data, 4, None) == _abi.E_INVAL
    assert _abi.lib().cls_addr_classes(None, 2, lo.ctypes.data, 4, C.byref(cnt)) == _abi.E_INVAL
    assert (lo == 9).all() and cnt.value == 9
    assert _abi.lib().cls_addr_classes(None, 0, lo.ctypes.data, 4, C.byref(cnt)) == 0
    assert cnt.value == 1 and lo.tolist() == [0, 9, 9, 9]
    # a cap too small sets only the count; no buffer at all likewise
    from vpp_amd import model as M
    cr = _abi.CRules([M.icmp_rule(M.PERMIT, "10.1.0.0/16", "192.168.7.9/32")])
    lo[:] = 9
    assert _abi.lib().cls_addr_classes(cr.ptr(), cr.n, lo.ctypes.data, 3, C.byref(cnt)) == 0
    assert cnt.value == 5 and (lo == 9).all()
    assert _abi.lib().cls_addr_classes(cr.ptr(), cr.n, None, 0, C.byref(cnt)) == 0 and cnt.value == 5
    five = np.zeros(5, np.uint32)
    assert _abi.lib().cls_addr_classes(cr.ptr(), cr.n, five.ctypes.data, 5, C.byref(cnt)) == 0
    assert five.tolist() == [0, 0x0A010000, 0x0A020000, 0xC0A80709, 0xC0A8070A]


def _layout(struct, fields):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "contivcls.h"\nint main(void) {\n'
           'printf("%%zu", sizeof(%s));\n' % struct +
           "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) +
           'printf(" %u %u", (unsigned)CLS_EXT_EGRESS, (unsigned)CLS_EXT_INGRESS);\nreturn 0; }\n')
    exe = os.path.join(ROOT, "go", "shimtest", "reach_ext_layout_cpu_check")
    try:
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-x", "c",
                            "-", "-o", exe], input=src, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    finally:
        if os.path.exists(exe):
            os.remove(exe)


@pytest.mark.parametrize("struct, ct", [("cls_addr_range", _abi.AddrRange), ("cls_reach_ext_out", _abi.ReachExtOut)])
def test_layouts_match_the_header(struct, ct):
    """Both structures as the C compiler lays them out (LP64): the ctypes
    structures' sizes and field offsets; the record is 16 bytes and the numpy
    dtype is the same record; the direction bits."""
    names = [f for f, _ in ct._fields_]
    got = _layout(struct, names)
    assert got[-2:] == [_abi.EXT_EGRESS, _abi.EXT_INGRESS] == [1, 2]
    got = got[:-2]
    assert got[0] == C.sizeof(ct)
    assert got[1:] == [getattr(ct, f).offset for f in names]
    if ct is _abi.AddrRange:
        assert got[0] == 16 and _abi.ADDR_RANGE.itemsize == 16
        assert [_abi.ADDR_RANGE.fields[f][1] for f in names] == got[1:]
        assert names == ["src", "probe", "dir", "action", "addr_lo", "addr_hi"]


def _acls():
    from aclgen import random_acl, random_acl16
    out = []
    for weird in (0.0, 0.003, 0.15):
        out.append(("random_acl %g" % weird, 4, random_acl(31, 300, weird=weird)[0]))
        out.append(("random_acl16 %g" % weird, 16, random_acl16(32, 300, weird=weird)[0]))
    return out


def test_the_adversarial_strings_are_there():
    """What the random ACLs must contain for the test below to mean
    something: unparsable strings, ::ffff:a.b.c.d/n with n above and below 96,
    /0 and /32 -- and what each contributes."""
    seen = set()
    for _, _, rules in _acls():
        seen.update(s for s in xc.rule_networks(rules) if s)
    assert {"garbage", "10.0.0.0/33", "::ffff:10.0.0.0/95", "::ffff:0:0/95", "::/0"} <= seen
    assert any(re.match(r"::ffff:[\d.]+/(9[6-9]|1[0-2]\d)$", s) for s in seen)
    assert any(re.match(r"[\d.]+/0$", s) for s in seen) and any(re.match(r"[\d.]+/32$", s) for s in seen)
    for s in ("garbage", "10.0.0.0/33", "10.0.0/8", "1.2.3.4", "::ffff:10.0.0.0/95", "::ffff:0:0/95", "::/0",
              "fd00:10::/64", ""):
        assert xc.net_interval(s) is None, s
    assert xc.net_interval("010.001.0.0/16") == (0x0A010000, 0x0A01FFFF)     # Go 1.9 reads the zeros as decimal
    assert xc.net_interval("0.0.0.0/0") == (0, 0xFFFFFFFF)
    assert xc.net_interval("9.9.9.9/0") == (0, 0xFFFFFFFF)
    assert xc.net_interval("255.255.255.255/32") == (0xFFFFFFFF, 0xFFFFFFFF)
    assert xc.net_interval("::ffff:10.1.2.3/120") == (0x0A010200, 0x0A0102FF)
    assert xc.net_interval("::ffff:10.1.2.3/96") == (0, 0xFFFFFFFF)
    assert xc.net_interval("10.1.2.3/31") == (0x0A010202, 0x0A010203)


def _ip(a, fam):
    return int(a).to_bytes(4, "big") if fam == 4 else b"\0" * 10 + b"\xff\xff" + int(a).to_bytes(4, "big")


def test_addr_classes_of_random_acls():
    """cls_addr_classes on random ACLs with adversarial network strings: the
    starts ascend from 0, each is 0, a network's lo or hi + 1, every network's
    interval holds whole classes, they equal the restatement -- and, exactness,
    the literal oracle's evalACL (action and terminating rule) is the same at
    the first, the last and a random interior address of every class, for
    several pod-side addresses and protocols, with the remote address as the
    source and as the destination."""
    import oracle
    from vpp_amd.engine import Engine
    rng = np.random.default_rng(5)
    most = 0
    for what, fam, rules in _acls():
        lo = Engine.addr_classes(rules)
        assert lo.dtype == np.uint32 and lo[0] == 0 and (np.diff(lo.astype(np.int64)) > 0).all(), what
        ok, ivs = xc.allowed_starts(rules)
        assert set(lo.tolist()) <= ok, (what, sorted(set(lo.tolist()) - ok)[:8])
        assert (xc.class_starts([rules]) == lo).all(), what
        most = max(most, len(lo))
        starts = lo.astype(np.int64)
        ends = np.append(starts[1:], xc.ALL32) - 1
        for a, b in set(ivs):                        # a network begins and ends on class boundaries
            assert a in starts and b in ends, (what, a, b)
        inner = starts + (rng.random(len(starts)) * (ends - starts + 1)).astype(np.int64)
        assert ((starts <= inner) & (inner <= ends)).all()
        # pod-side addresses: inside networks of the list, and anything
        pods = [_ip(ivs[i][0], fam) for i in rng.integers(0, len(ivs), 3)] + [_ip(0x08080808, fam)]
        if fam == 16:
            pods.append(bytes.fromhex("fd000010000000000000000000000001"))
        cr = oracle.rules_to_c(rules)
        for j, pod in enumerate(pods):
            proto, dport = ((0, 80), (1, 53), (2, 0), (0, 443), (47, 0))[j]
            for k in range(len(starts)):
                got = set()
                for a in (starts[k], ends[k], inner[k]):
                    rem = _ip(a, fam)
                    got.add((oracle.eval_acl(cr, False, rem, pod, proto, dport),
                             oracle.eval_acl(cr, False, pod, rem, proto, dport)))
                assert len(got) == 1, (what, k, int(starts[k]), int(ends[k]), got)
    assert most > 16                                 # (a pool of 24 prefixes: at most 49 starts)


def _rows(rec):
    return [(int(r["dir"]), int(r["probe"]), int(r["src"]), int(r["addr_lo"]), int(r["addr_hi"]), int(r["action"]))
            for r in rec]


def test_ranges_ref_on_hand_made_arrays():
    top = 0xFFFFFFFF
    # K = 1: one range per line, the whole space
    v = np.array([2, 0, 3, 2, 1, 2], np.uint8).reshape(2, 1, 3, 1)
    rec, total, runs, allow, hist = xc.ranges_ref(v, [0])
    assert total == 6 and rec.dtype == _abi.ADDR_RANGE and (runs == 1).all()
    assert _rows(rec) == [(0, 0, 0, 0, top, 2), (0, 0, 1, 0, top, 0), (0, 0, 2, 0, top, 3), (1, 0, 0, 0, top, 2),
                          (1, 0, 1, 0, top, 1), (1, 0, 2, 0, top, 2)]
    assert allow.dtype == np.uint64 and allow.tolist() == [[[2 ** 32, 0, 0]], [[2 ** 32, 0, 2 ** 32]]]
    assert hist.dtype == np.uint64 and hist.tolist() == [[[2 ** 32, 0, 2 ** 32, 2 ** 32]], [[0, 2 ** 32, 2 ** 33, 0]]]
    # one direction, two probes, two endpoints; the last class starts at 0xFFFFFFFF, one at 1
    starts = [0, 1, 100, 200, top]
    v = np.zeros((1, 2, 2, 5), np.uint8)
    v[0, 0, 0] = [2, 2, 2, 2, 2]                       # a single range
    v[0, 0, 1] = [0, 2, 2, 2, 2]                       # a change at 0 -> 1
    v[0, 1, 0] = [0, 0, 0, 0, 3]                       # a change at 0xFFFFFFFE -> 0xFFFFFFFF
    v[0, 1, 1] = [0, 0, 2, 1, 1]
    rec, total, runs, allow, hist = xc.ranges_ref(v, starts, dirs=[1])
    assert total == 8
    assert _rows(rec) == [(1, 0, 0, 0, top, 2), (1, 0, 1, 0, 0, 0), (1, 0, 1, 1, top, 2), (1, 1, 0, 0, top - 1, 0),
                          (1, 1, 0, top, top, 3), (1, 1, 1, 0, 99, 0), (1, 1, 1, 100, 199, 2), (1, 1, 1, 200, top, 1)]
    assert runs.tolist() == [[[1, 2], [2, 3]]] and runs.dtype == np.uint32
    assert allow.tolist() == [[[2 ** 32, 2 ** 32 - 1], [0, 100]]]
    assert hist.tolist() == [[[1, 0, 2 ** 33 - 1, 0], [2 ** 32 - 1 + 100, 2 ** 32 - 200, 100, 1]]]
    assert (hist.sum(axis=2) == 2 * 2 ** 32).all()
    # the same verdicts on a finer decomposition: equal neighbours merge
    fine = [0, 1, 2, 50, 100, 150, 200, 4000, top - 1, top]
    at = np.searchsorted(starts, fine, side="right") - 1
    got = xc.ranges_ref(v[..., at], fine, dirs=[1])
    assert got[1] == total and got[0].tobytes() == rec.tobytes()
    assert (got[2] == runs).all() and (got[3] == allow).all() and (got[4] == hist).all()
    # cap cuts the records, not the total
    rec3, total3, _, _, _ = xc.ranges_ref(v, starts, cap=3, dirs=[1])
    assert total3 == 8 and rec3.tobytes() == rec[:3].tobytes()
    # lookup
    line = np.array([0, 1, 1, 2, 2, 3, 3, 3])
    addr = np.array([77, 0, 1, top - 1, top, 99, 100, top])
    assert xc.lookup(rec, line, addr, p=2, n=2, nd=1).tolist() == [2, 0, 2, 0, 3, 0, 2, 1]


@functools.lru_cache(maxsize=None)
def _case_ref(fam):
    starts = xc.class_starts(list(rc.case(fam)["by_name"].values()))
    return starts, xc.ranges_ref(xc.oracle_at(fam, [0, 1], np.arange(rc.N_EP), starts), starts)


@pytest.mark.parametrize("fam", [4, 16])
def test_the_case_is_not_degenerate(fam):
    """All 37 endpoints x 3 probes x both directions through `if0`, on the
    oracle alone: enough classes, every ConnectionAction in each direction,
    lines with one range and lines with many."""
    c = rc.case(fam)
    starts, (rec, total, runs, allow, hist) = _case_ref(fam)
    bound = xc.class_starts(xc.bound_rules(c, np.arange(rc.N_EP)))
    assert len(starts) >= len(bound) >= 100 and np.isin(bound, starts).all()
    assert runs.shape == (2, 3, rc.N_EP) and total == runs.sum()
    for d in (0, 1):
        assert set(rec["action"][rec["dir"] == d].tolist()) == {0, 1, 2, 3}
        assert (hist[d] > 0).any(axis=0).all()
        assert runs[d].min() == 1 and runs[d].max() >= 32
    assert (hist.sum(axis=2) == 2 ** 32 * rc.N_EP).all() and (allow <= 2 ** 32).all()
    # the bound ACLs' classes alone give the same ranges
    at = xc.ranges_ref(xc.oracle_at(fam, [0, 1], np.arange(rc.N_EP), bound), bound)
    assert at[1] == total and at[0].tobytes() == rec.tobytes() and (at[4] == hist).all()


def test_ext_shims_compile_as_c99():
    """contivcls_go.h with the external-sweep shims, and go/shimtest/reachext.c
    that calls them, as strict C99 (gcc -std=c99 -Werror), linked to the
    library."""
    hdr = open(os.path.join(ROOT, "include", "contivcls_go.h")).read()
    assert "clsg_reach_external_v4(" in hdr and "clsg_reach_external_v16(" in hdr
    out = os.path.join(ROOT, "go", "shimtest", "reachext_cpu_check")
    try:
        r = subprocess.run(["gcc", "-O1", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                            "-I" + os.path.join(ROOT, "include"), "-o", out,
                            os.path.join(ROOT, "go", "shimtest", "reachext.c"),
                            "-L" + os.path.join(ROOT, "vpp_amd"), "-lcontivcls",
                            "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    finally:
        if os.path.exists(out):
            os.remove(out)
    mk = open(os.path.join(ROOT, "go", "shimtest", "Makefile")).read()
    assert re.search(r"^all:.*\$\(HERE\)reachext\b", mk, re.M) and re.search(r"rm -f .*\$\(HERE\)reachext\b", mk)


def test_go_binding_calls_the_ext_shims_with_go19_api():
    from test_go_binding_cpu import POST_19, _code
    code = _code(GO)
    assert "C.clsg_reach_external_v4(" in code and "C.clsg_reach_external_v16(" in code
    assert "func (en *Engine) ReachExternal(" in code
    # only through the shims: neither the entry point nor its structures
    assert "C.cls_reach_external" not in code and "C.cls_addr_range" not in code
    for pat in POST_19:
        assert not re.search(pat, code), pat
