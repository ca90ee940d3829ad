"""CPU: the connection trace's boundary (cls_connect_rules, the trace twin of
cls_connect_batch) and the oracle-only preconditions of its GPU tests.

The trace reports, per connection, the rule at which each of testConnection's
four evalACL calls ended (aclengine_mock.go:394-471, the matched rule logged at
:651-654); its definition is orc_test_connection_hits' hits[4].  Here: the
header declares the entry point and the library exports it, it refuses a null
engine and CLS_F_COUNT without a device, the Go shims exist -- and the
workloads tests/test_gpu_connect_trace.py runs are rich enough that an exact
match there means something: every verdict, every call position with
default-DENY and rule entries, many distinct (position, rule) pairs, rows of
four -1 and rows of four calls, and (the large-ACL workloads) calls ending on
many rules of the global table.

The workloads (and their oracle rows) are computed once per process and shared
with the GPU tests, which import them from here.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import oracle
from test_gpu_connect_scale import _addr, build, traffic
from vpp_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder:
    """Stands in for an engine in test_gpu_connect_scale.build: records the
    ACLs instead of installing them (install() replays them on an engine)."""

    def __init__(self):
        self.acls = []

    def acl_put(self, name, rules, ing, eg):
        self.acls.append((name, rules, list(ing), list(eg)))
        return 0

    def install(self, eng):
        for name, rules, ing, eg in self.acls:
            assert eng.acl_put(name, rules, ing, eg) == 0


def oracle_rows(bind, by_name, ifs, si, di, tr, fam):
    """(verdicts uint8[n], rows int32[n, 4]) of orc_test_connection_hits: row i
    = the terminating rules of connection i's evalACL calls in call order (src
    inbound, dst outbound, dst inbound, src outbound), R = default DENY, -1 =
    not made or a nil ACL."""
    crs = {name: oracle.rules_to_c(rules) for name, rules in by_name.items()}
    refs = {None: oracle.AclRef(None, 0, 1)}
    for name, cr in crs.items():
        refs[name] = oracle.AclRef(cr.ptr(), cr.n, 0)
    L = oracle.lib()
    n = len(tr["proto"])
    out = np.zeros(n, np.uint8)
    rows = np.zeros((n, 4), np.int32)
    hits = (C.c_int32 * 4)()
    alen = 4 if fam == 4 else 16
    for i in range(n):
        a, b = ifs[si[i]], ifs[di[i]]
        s, d = _addr(tr["src"][i], fam), _addr(tr["dst"][i], fam)
        rc = L.orc_test_connection_hits(C.byref(refs[bind[a][0]]), C.byref(refs[bind[a][1]]),
                                        C.byref(refs[bind[b][0]]), C.byref(refs[bind[b][1]]), 1 if a == b else 0,
                                        s, alen, d, alen, int(tr["proto"][i]), int(tr["sport"][i]),
                                        int(tr["dport"][i]), hits)
        assert rc >= 0
        out[i] = rc
        rows[i] = hits[:]
    return out, rows


def call_acls(w):
    """[n][4] ACL name (or None) of each call position of the workload's
    connections: src inbound, dst outbound, dst inbound, src outbound."""
    ifs, bind = w["ifs"], w["bind"]
    return [(bind[ifs[a]][0], bind[ifs[b]][1], bind[ifs[b]][0], bind[ifs[a]][1]) for a, b in zip(w["si"], w["di"])]


@functools.lru_cache(maxsize=None)
def workload(seed, fam, n_local, n_if=80, n=20000, cfg=2):
    """build(seed, n_local, n_if, cfg, fam) and traffic(seed, ...) of
    test_gpu_connect_scale with the interfaces drawn as its _run draws them,
    and the oracle's verdicts and rows.  Shared: nothing in it may be written."""
    rec = Recorder()
    ifs, bind, by_name, pool, spec = build(rec, seed, n_local=n_local, n_if=n_if, cfg=cfg, fam=fam)
    tr = traffic(seed, n, pool, spec, fam)
    rng = np.random.default_rng(seed)
    si = rng.integers(0, len(ifs), n)
    di = np.where(rng.random(n) < 0.1, si, rng.integers(0, len(ifs), n))
    verdict, rows = oracle_rows(bind, by_name, ifs, si, di, tr, fam)
    for x in (si, di, verdict, rows, *tr.values()):
        x.setflags(write=False)
    return {"rec": rec, "ifs": ifs, "bind": bind, "by_name": by_name, "pool": pool, "spec": spec, "tr": tr,
            "si": si, "di": di, "verdict": verdict, "rows": rows, "fam": fam}


# (seed, fam, locals) of the trace's GPU workloads, n_if = 80
WORKLOADS = [(0, 4, 64), (1, 4, 12), (0, 16, 64), (1, 16, 12)]
# ... and of its large-ACL cases (mode "classifier"), n_if = 24: the global
# table on 3 of 24 interfaces
LARGE = [(0, 4, 12), (0, 16, 12)]
LARGE_N_IF = 24


def header(name="contivcls.h"):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_and_library_exports_connect_rules():
    assert re.search(r"^int\s+cls_connect_rules\s*\(\s*cls_engine\*\s*e,\s*const cls_conn_soa\*\s*conns,\s*uint64_t n,"
                     r"\s*uint8_t\*\s*conn_verdict_out,\s*int32_t\*\s*rule_out,\s*uint32_t flags,\s*void\*\s*stream\)",
                     header(), re.M)
    assert "cls_connect_rules" in _abi.SYMBOLS
    assert hasattr(_abi.lib(), "cls_connect_rules")
    # additive: the ABI version and the flag set stay (tests/test_abi.py pins both)
    assert _abi.lib().cls_abi_version() == 5


def test_connect_rules_refuses_null_engine_and_counting_without_a_device():
    """CLS_E_INVAL before any device call: a null engine, null connections, a
    missing rule_out, and CLS_F_COUNT (the trace touches no counters)."""
    L = _abi.lib()
    cs = _abi.ConnSoa(_abi.PktSoa(_abi.AF_V4, None, None, None, None, None, None, None), None, None)
    rules = (C.c_int32 * 4)()
    out = (C.c_uint8 * 1)()
    assert L.cls_connect_rules(None, C.byref(cs), 0, out, rules, 0, None) == _abi.E_INVAL
    assert L.cls_connect_rules(None, C.byref(cs), 1, out, rules, _abi.F_COUNT, None) == _abi.E_INVAL
    assert L.cls_connect_rules(None, None, 0, None, None, 0, None) == _abi.E_INVAL
    # (CLS_F_COUNT on a real engine: test_gpu_connect_trace.py)


def test_go_header_defines_both_trace_shims():
    text = header("contivcls_go.h")
    for shim in ("clsg_connect_rules_v4", "clsg_connect_rules_v16"):
        m = re.search(r"static inline int %s\s*\(([^)]*)\)\s*\{(.*?)\n\}" % shim, text, re.S)
        assert m, shim
        assert "int32_t* rules" in m.group(1) and "cls_connect_rules(e, &c, n, out, rules, flags, NULL)" in m.group(2)
    go = open(os.path.join(ROOT, "go", "contivcls", "contivcls.go")).read()
    assert "C.clsg_connect_rules_v4(" in go and "C.clsg_connect_rules_v16(" in go
    assert "C.cls_connect_rules(" not in go          # only through the shims (no SoA record built in Go)


@pytest.mark.parametrize("seed,fam,n_local", WORKLOADS)
def test_trace_workloads_exercise_every_call_position(seed, fam, n_local):
    """The oracle alone: an exact match on these 20,000 connections covers all
    four verdicts, every call position with default-DENY and rule entries,
    many (position, rule) pairs, untraced rows and fully traced rows."""
    w = workload(seed, fam, n_local)
    v, rows = w["verdict"], w["rows"]
    acls = call_acls(w)
    n_rules = np.array([[len(w["by_name"][x]) if x else -1 for x in row] for row in acls])
    made = rows >= 0
    dflt = made & (rows == n_rules)
    print("verdicts", np.bincount(v, minlength=4).tolist(), "calls", made.sum(0).tolist(), "default DENY",
          dflt.sum(0).tolist(), "distinct", len({(k, int(r)) for k in range(4) for r in rows[made[:, k], k]}),
          "all -1", int((~made).all(1).sum()), "four calls", int(made.all(1).sum()))
    assert set(v.tolist()) == {0, 1, 2, 3}
    assert (rows[made] <= n_rules[made]).all()
    for k in range(4):
        assert made[:, k].sum() >= 1000, k
        assert dflt[:, k].sum() >= 300, k
        assert (made[:, k] & ~dflt[:, k]).sum() >= 700, k
    assert len({(k, int(r)) for k in range(4) for r in rows[made[:, k], k]}) >= 150
    assert (~made).all(1).sum() >= 400
    assert made.all(1).sum() >= 10


@pytest.mark.parametrize("seed,fam,n_local", LARGE)
def test_large_acl_workloads_reach_the_global_table(seed, fam, n_local):
    """The oracle alone, the large-ACL cases (24 interfaces): >= 500 traced
    calls land on the global table and reach >= 10 distinct rules of it."""
    w = workload(seed, fam, n_local, n_if=LARGE_N_IF)
    acls = call_acls(w)
    on_global = np.array([[x == "global" for x in row] for row in acls]) & (w["rows"] >= 0)
    rules = set(w["rows"][on_global].tolist())
    print("calls on global", int(on_global.sum()), "distinct rules", len(rules))
    assert on_global.sum() >= 500
    assert len(rules) >= 10
