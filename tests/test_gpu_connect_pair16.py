"""The 16-byte connection pair launch on the GPU (classify16_pair,
vpp_amd/csrc/k16_pair.hip; option conn_pair16).

A mixed-family connection batch (CLS_AF_V16) evaluates each large ACL for
both tuples of every connection in one launch on the table's pair image
(compile.hpp build_pair16: the 16-byte image with a fourth cell per source
class for protocols > 2) and hands the connection kernel one result byte per
connection, or u16 / u32 counter-index words when the batch counts.  Every
test passes conn_pair16 itself, so the file holds whichever default the
option has.  Verdicts and per-(ACL, rule) counters are bit-exact against
orc_test_connection_hits (the oracle of test_gpu_connect_scale, whose
builders these tests reuse), or, for the tail sizes, against the pure-scan
mode of the same engine.  The engine's debug_conn lines say which launch a
large ACL took: ``pair16: pimg ...`` the pair launch (with its front end,
``fe``, the size of the slot -> rule map staged in LDS, ``map``, the grid and
the connections per wave-step), ``slots16: ...`` the two slot launches.
"""
import re

import numpy as np
import pytest

from aclgen import mix_families, random_acl16, random_traffic, single_port_acl
from test_gpu_connect_scale import build, oracle_connections, traffic

pytestmark = pytest.mark.gpu


class _Recorder:
    """build()'s engine when only the ACLs and bindings are wanted."""

    def acl_put(self, *_a):
        return 0


def _dev(x):
    import torch
    x = np.ascontiguousarray(x)
    if x.ndim == 2:
        return torch.from_numpy(x).to("cuda")
    return torch.from_numpy(x.view({4: np.int32, 2: np.int16, 1: np.uint8}[x.dtype.itemsize])).to("cuda")


def _lines(capfd):
    err = capfd.readouterr().err.splitlines()
    return [ln for ln in err if ln.startswith("pair16:")], [ln for ln in err if ln.startswith("slots16:")]


class _Case:
    """ACLs, bindings, connections and the oracle's verdicts and counters:
    computed once, shared (unchanged) by the tests of one setup."""

    def __init__(self, seed, n, cfg=2, n_local=6, n_if=16, extra=None, hot=None):
        self.seed, self.cfg, self.n_local, self.n_if = seed, cfg, n_local, n_if
        self.extra = extra or []                      # (name, rules, ingress, egress) after build()'s ACLs
        ifs, bind, by_name, pool, spec = build(_Recorder(), seed, n_local=n_local, n_if=n_if, cfg=cfg, fam=16)
        for name, rules, ing, eg in self.extra:
            by_name[name] = rules
            for i in ing + eg:
                if i not in bind:
                    ifs.append(i)
                    bind[i] = [None, None]
            for i in ing:
                bind[i][0] = name
            for i in eg:
                bind[i][1] = name
        self.ifs, self.bind, self.by_name = ifs, bind, by_name
        tr = traffic(seed, n, pool, spec, 16)
        rng = np.random.default_rng(seed)
        other = rng.random(n) < 0.05
        other[-3:] = True                             # the per-connection tail too
        tr["proto"] = np.where(other, 47, tr["proto"]).astype(np.uint8)
        self.tr, self.n = tr, n
        # sources on the large ACLs' interfaces: their words decide
        hot = np.arange(3) if hot is None else np.array([ifs.index(x) for x in hot])
        self.si = rng.choice(hot, n)
        self.di = rng.integers(0, len(ifs), n)
        self._want = None

    def want(self):
        if self._want is None:
            self._want = oracle_connections(self.bind, self.by_name, self.ifs, self.si, self.di, self.tr, 16)
        return self._want

    def install(self, eng):
        build(eng, self.seed, n_local=self.n_local, n_if=self.n_if, cfg=self.cfg, fam=16)
        for name, rules, ing, eg in self.extra:
            assert eng.acl_put(name, rules, ing, eg) == 0
        ids = np.array([eng.if_id(x) for x in self.ifs], np.uint32)
        tr = self.tr
        return [ids[self.si], ids[self.di], tr["src"], tr["dst"], tr["proto"], tr["sport"], tr["dport"]]

    def check(self, eng, args, mode, count, n=None):
        n = self.n if n is None else n
        if mode == "device":
            import torch
            dv = [_dev(x[:n]) for x in args]
            torch.cuda.synchronize()
            got = eng.connect_batch(*dv, mode="classifier", count=count).cpu().numpy()
        else:
            got = eng.connect_batch(*[x[:n] for x in args], mode=mode, count=count)
        want, wcounts = self.want()
        bad = np.nonzero(got != want[:n])[0]
        assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]])
        if count:
            assert n == self.n
            for name in self.by_name:
                c = eng.conn_counters(name, reset=True)
                d = np.nonzero(c != wcounts[name])[0]
                assert d.size == 0, (name, d[:10], c[d[:10]], wcounts[name][d[:10]])
        return got


@pytest.fixture(scope="module")
def case2():
    """The config-2 twin as global ACL, 6 locals, 16 interfaces, 16003
    connections (5 % protocol 47, the last three included) whose sources sit
    on the global ACL's interfaces."""
    c = _Case(21, 16003)
    assert len(set(c.want()[0].tolist())) >= 3       # allowed, denied, reflected / failure all seen
    assert sum(int(v.sum()) for v in c.want()[1].values()) > c.n // 4
    return c


def _engine(**opts):
    from vpp_amd.engine import Engine
    return Engine(options=dict(opts, debug_conn=1))


@pytest.mark.parametrize("count", [False, True])
@pytest.mark.parametrize("mode", ["classifier", "device"])
@pytest.mark.parametrize("pair16", [1, 0])
def test_pair16_launch_matches_oracle(case2, pair16, mode, count, capfd):
    """Every large ACL of the batch on the pair launch (no slot launches), or
    (conn_pair16=0) none: the same verdicts and counters."""
    eng = _engine(conn_pair16=pair16)
    try:
        args = case2.install(eng)
        capfd.readouterr()
        case2.check(eng, args, mode, count)
    finally:
        eng.close()
    pair, slots = _lines(capfd)
    if pair16:
        assert pair and all(ln.startswith("pair16: pimg ") for ln in pair) and not slots, (pair, slots)
        assert any(" fe 1 " in ln for ln in pair), pair          # the global table: host-route hashes
        if count:                                                # counter indices from the map in LDS
            assert all(" map 0 " not in ln for ln in pair), pair
    else:
        assert slots and not pair, (pair, slots)


@pytest.mark.parametrize("opts,count,paired", [({"conn_pre_narrow": 0}, False, True),
                                               ({"conn_pre_narrow": 0}, True, True),
                                               ({"pair_map_lds": 0}, True, True),
                                               ({"conn_pre_rules": 0}, True, False),
                                               ({"conn_pre_rules": 0}, False, True)])
def test_pair16_output_formats(case2, opts, count, paired, capfd):
    """u32 words instead of result bytes / u16 counter-index words
    (conn_pre_narrow=0), the slot -> rule map gathered from global memory
    (pair_map_lds=0), and a counting batch without counter-index words
    (conn_pre_rules=0), which keeps the two slot launches."""
    eng = _engine(conn_pair16=1, **opts)
    try:
        args = case2.install(eng)
        capfd.readouterr()
        case2.check(eng, args, "classifier", count)
    finally:
        eng.close()
    pair, slots = _lines(capfd)
    if not paired:
        assert slots and not pair, (pair, slots)
        return
    assert pair and not slots, (pair, slots)
    if opts.get("pair_map_lds") == 0 or not count:
        assert all(" map 0 " in ln for ln in pair), pair


def _front_case(kind):
    if kind == "trie":
        rules, pool = single_port_acl(3, 200)
        rules, _ = mix_families(rules, random_traffic(1, 4, pool), 3)
    else:
        rules, _ = random_acl16(7300, 300, 0.05)
    return _Case(33, 6000, n_local=3, n_if=10, extra=[("front", rules, ["f0", "f1"], ["f1", "f2"])],
                 hot=["f0", "f1", "f2"])


_FRONT = {}


@pytest.mark.parametrize("kind,opts,fe", [("search", {"v16_src_search": 1}, 0), ("trie", {"v16_src_trie": 1}, 2),
                                          ("dst", {"orient": "dst", "v16_src_search": 1}, 0),
                                          ("core_search", {"v16_src_search": 1, "src_search": 1, "trie": 0}, 0)])
@pytest.mark.parametrize("count", [False, True])
def test_pair16_front_ends_and_orientation(kind, opts, fe, count, capfd):
    """A large local ACL where most connections reach it: the interval-search
    front end (src_mode 0: reps through the core's own source lookup -- its
    hash LPM or trie as compiled, or the interval search, core_search), the
    IPv4 source trie (src_mode 2) and a destination-keyed image."""
    key = "trie" if kind == "trie" else "random"
    if key not in _FRONT:
        _FRONT[key] = _front_case(key)
    case = _FRONT[key]
    eng = _engine(conn_pair16=1, **opts)
    try:
        args = case.install(eng)
        capfd.readouterr()
        case.check(eng, args, "classifier", count)
    finally:
        eng.close()
    pair, slots = _lines(capfd)
    assert pair and not slots, (pair, slots)
    assert any(" fe %d " % fe in ln for ln in pair), pair
    if kind != "trie":                                # (the global table keeps its hashes unless the search is forced)
        assert all(" fe 0 " in ln for ln in pair), pair


def test_pair16_tail_sizes_match_linear(case2, capfd):
    """Batches smaller than a wave-step, one connection past whole steps,
    and an odd number of them: the per-connection tail gives the vector
    path's words."""
    eng = _engine(conn_pair16=1)
    try:
        args = case2.install(eng)
        capfd.readouterr()
        for n in (1, 3, 255, 259, 1027):
            got = eng.connect_batch(*[x[:n] for x in args], mode="classifier")
            lin = eng.connect_batch(*[x[:n] for x in args], mode="linear")
            assert np.array_equal(got, lin), n
            assert np.array_equal(got, case2.want()[0][:n]), n
    finally:
        eng.close()
    pair, slots = _lines(capfd)
    assert pair and not slots, (pair, slots)


def test_pair16_partial_last_step_matches_linear(case2, capfd):
    """Two steps per lane, the second taken by a prefix of the grid's waves
    only (the others hold a prefetch they never use), then a tail: sized from
    the launch's own grid and connections per wave-step."""
    import torch
    eng = _engine(conn_pair16=1)
    try:
        args = case2.install(eng)
        eng.connect_batch(*[x[:4096] for x in args], mode="classifier")
        pair, _ = _lines(capfd)
        step = int(re.search(r" step (\d+)", pair[0]).group(1))
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        waves = cus * 16                              # one 1024-thread workgroup per CU
        n = 2 * waves * step - 21 * step - 5
        reps = -(-n // case2.n)
        big = [np.concatenate([x] * reps)[:n] for x in args]
        got = eng.connect_batch(*big, mode="classifier")
        pair, slots = _lines(capfd)
        grid = int(re.search(r" grid (\d+)", pair[0]).group(1))
        assert pair and not slots and waves * step < n < 2 * waves * step and grid == cus, (pair, slots, n, cus)
        want = eng.connect_batch(*big, mode="linear")
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]])
    finally:
        eng.close()


@pytest.mark.parametrize("count", [False, True])
def test_pair16_two_large_acls(count, capfd):
    """Two large 16-byte ACLs (the config-2 twin and a 300-rule random one on
    interfaces of their own, most connections through both): a pair block
    each."""
    if "two" not in _FRONT:
        big2, _ = random_acl16(4242, 300, 0.0)
        _FRONT["two"] = _Case(13, 12000, n_local=3, n_if=12, extra=[("big2", big2, ["bx0", "bx1"], ["bx1", "bx2"])],
                              hot=["if0", "if1", "if2", "bx0", "bx1", "bx2"])
    case = _FRONT["two"]
    eng = _engine(conn_pair16=1)
    try:
        args = case.install(eng)
        capfd.readouterr()
        case.check(eng, args, "classifier", count)
        if count:
            _, wcounts = case.want()
            assert wcounts["big2"].sum() > 1000 and wcounts["global"].sum() > 1000
    finally:
        eng.close()
    pair, slots = _lines(capfd)
    assert len(pair) >= 2 and not slots, (pair, slots)


def test_pair16_falls_back_when_the_pair_image_does_not_fit(capfd):
    """The config-3 twin (a 163 KB main image in list mode 0): its four-cell
    image does not fit LDS, so the table keeps the two slot launches."""
    case = _Case(4, 12000, cfg=3, n_local=2, n_if=10)
    assert all(len(r) < 64 for name, r in case.by_name.items() if name != "global")   # one large ACL
    eng = _engine(conn_pair16=1)
    try:
        args = case.install(eng)
        capfd.readouterr()
        case.check(eng, args, "classifier", False)
    finally:
        eng.close()
    pair, slots = _lines(capfd)
    assert slots and not pair, (pair, slots)
