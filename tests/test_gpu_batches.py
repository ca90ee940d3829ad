"""Engine-owned batches (vpp_amd/csrc/fleet.cpp: cls_batch_*,
cls_classify_batch, cls_batch_connect) in the 16-byte layout and at the
edges of their shards, bit-exact against the oracle (oracle.classify_fast,
gen_traffic_v16 / v4, orc_test_connection_hits) or, for pure data movement,
against a numpy model of the batch (tests/batch_cases.py).

Shards: a device list repeating device 0 (G peer engines on the one GPU of
the box: no communicator, counters summed on the host), and a one-device
engine with cls_comm_init (an RCCL group of one: the all-reduce path).  Each
test asserts the precondition that puts it on the branch it is about.

 1. the 16-byte and IPv4 generators into ragged shards (`+ s.first`), every
    input field read back, CLS_BF_SPORT included
 2. 16-byte classify: uploaded through Batch.upload, verdicts and merged
    counters; whole grid steps on one device; CLS_F_FORCE_LINEAR,
    CLS_F_NO_VERDICT, CLS_F_ACCUMULATE through cls_classify_batch
 3. 16-byte connection batches on four shards (classify16_pair or the two
    slot launches), counted once; every shard's engine sees the options
 4. a rebind (equal rules put again) clears every shard's counters
 5. shards that are empty or shorter than a vector group, n = 0
 6. upload / download windows across shard boundaries at every element
    width, to and from the mirror at first != 0; the refusals
 7. three staging chunks from pageable memory (buffer 0 reused)
 8. two tables of different size on one batch: the counter buffers grow
 9. options set on the primary reach the peers
10. two distinct devices (skipped on a one-GPU box)
"""
import numpy as np
import pytest

import oracle
from batch_cases import (CONN_IFS, CONN_LOCALS, CONN_SEED, EDGE_NS, FIELDS16, INPUTS, N, N_CHUNKED, STAGE_BYTES,
                         BatchModel, batch4, batch16, bound_interfaces, case16, classify_ref, conn_case, crosses,
                         random_field, shard_starts, stage_chunks, table16, two_tables, windows)
from vpp_amd import _abi, workload
from vpp_amd._abi import AF_V4, AF_V16, ClsError
from vpp_amd.engine import Engine, Table, shard_range

pytestmark = pytest.mark.gpu

CONN_FIELDS = INPUTS + ((_abi.BF_SRC_IF, "sif"), (_abi.BF_DST_IF, "dif"))


def _engine(kind):
    """kind: a shard count G (device 0 listed G times; no communicator), or
    "comm1" (one device with an RCCL group of one)."""
    if kind == "comm1":
        eng = Engine(0)
        eng.comm_init()
        assert eng.comm_info() == (1, 0)
        return eng
    eng = Engine(devices=[0] * kind)
    assert eng.n_devices() == kind and eng.comm_info() == (0, 0)
    return eng


def _n_shards(kind):
    return 1 if kind == "comm1" else kind


def _upload(b, tr, fields=INPUTS):
    for f, k in fields:
        b.upload(f, tr[k])


def _same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size:
        bad = np.nonzero((got != want).reshape(len(want), -1).any(1))[0]
        assert bad.size == 0, (what, bad.size, bad[:10], got[bad[:10]], want[bad[:10]])


def _last_error(eng) -> str:
    return _abi.lib().cls_last_error(eng.h).decode()


# ---- 1: the generators into shards ----------------------------------------

@pytest.fixture(scope="module")
def gen_refs():
    out = {}
    for af, cfg, gen in ((AF_V16, 5, oracle.gen_traffic_v16), (AF_V4, 3, oracle.gen_traffic_v4)):
        spec = workload.config(cfg)[1]
        out[af] = (spec, gen(spec, 777, N))
    return out


@pytest.mark.parametrize("G", [1, 3, 8])
@pytest.mark.parametrize("af", [AF_V16, AF_V4])
def test_generator_into_shards(gen_refs, af, G):
    """cls_batch_gen_traffic_v16 / v4: shard g generates stream packets
    [777 + first_g, ...) -- all five input fields of the whole batch equal
    the oracle's stream from 777 on (config 5's spec, config 3's for IPv4)."""
    spec, ref = gen_refs[af]
    eng = Engine(devices=[0] * G)
    try:
        b = eng.batch(N, af=af)
        assert [(s[1], s[2]) for s in b.shards()] == shard_starts(N, G)
        assert G == 1 or any(s[1] % 4 for s in b.shards())           # shard starts off the vector groups
        b.gen_traffic(spec, stream_first=777)
        for f, k in INPUTS:
            _same(b.download(f), ref[k], k)
    finally:
        eng.close()


# ---- 2: 16-byte classify through a batch ----------------------------------

@pytest.fixture(scope="module")
def single16():
    """Engine.classify (host arrays, one device) of case 2's batch."""
    rules, tr, ov, oc = case16()
    eng = Engine(0)
    try:
        t = eng.put_table("t16", rules)
        assert t.info()["has_v16"] == 1
        return eng.classify(t, tr["src"], tr["dst"], tr["dport"], tr["proto"])
    finally:
        eng.close()


def _classify16(eng, single=None):
    rules, tr, ov, oc = case16()
    assert (tr["proto"] == 47).any() and (tr["src"][:, :4] == (0xFD, 0, 0, 0x30)).all(1).any()
    t = eng.put_table("t16", rules)
    b = eng.batch(N, af=AF_V16)
    _upload(b, tr)
    b.upload(_abi.BF_VERDICT, np.full(N, 0xEE, np.uint8))
    c = eng.classify_batch(t, b)
    v = b.download(_abi.BF_VERDICT)
    _same(v, ov, "verdicts")
    _same(c, oc, "counters")
    assert int(c.sum()) == N and len(set(ov.tolist())) >= 3
    if single is not None:
        _same(v, single[0], "verdicts, one device")
        _same(c, single[1], "counters, one device")
    # the other counter buffer, enqueued only, read later
    assert eng.classify_batch(t, b, counters=False) is None
    _same(b.counters(t.n_rules), oc, "counters read later")
    return t, b


@pytest.mark.parametrize("kind", [3, 8, "comm1"])
def test_classify16_uploaded_batch(single16, kind):
    """300 random mixed-family rules (5 % odd ones) over IPv4-mapped and
    fd00:30::/96 packets with protocol 47 among them, uploaded field by field
    (16-byte elements through batch_move): every shard's verdicts and the
    merged counters equal the oracle's and one device's Engine.classify."""
    eng = _engine(kind)
    try:
        t, b = _classify16(eng, single16)
        assert [(s[1], s[2]) for s in b.shards()] == shard_starts(N, _n_shards(kind))
    finally:
        eng.close()


def test_classify16_whole_grid_steps():
    """One device, a batch large enough for whole grid steps of
    classify16_cls: a lane takes four packets a step and a CU holds at most
    2048 lanes (cls_grid: at most 2048 / block workgroups per CU), so the
    grid has at most 2048 n_cu lanes and n = 4 * 2048 * n_cu + 7 gives every
    lane a full step (n / 4 >= the grid's threads) and leaves a ragged rest
    (256 CUs: 2,097,159 packets)."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 4 * 2048 * n_cu + 7
    assert n // 4 >= 2048 * n_cu and n % 4
    rules, _ = table16()
    tr = batch16(n, 6)
    ov, oc = classify_ref(rules, tr, 16)
    eng = Engine(0)
    try:
        t = eng.put_table("t16", rules)
        b = eng.batch(n, af=AF_V16)
        _upload(b, tr)
        c = eng.classify_batch(t, b)
        _same(b.download(_abi.BF_VERDICT), ov, "verdicts")
        _same(c, oc, "counters")
    finally:
        eng.close()


@pytest.mark.parametrize("kind", [3, "comm1"])
def test_classify16_batch_flags(kind):
    """cls_classify_batch's flags through the C ABI: CLS_F_FORCE_LINEAR gives
    the classifier's result; CLS_F_NO_VERDICT leaves CLS_BF_VERDICT as it was
    (a 0xEE sentinel) with exact counters; CLS_F_ACCUMULATE adds to the
    caller's vector."""
    L = _abi.lib()
    rules, tr, ov, oc = case16()
    eng = _engine(kind)
    try:
        t = eng.put_table("t16", rules)
        b = eng.batch(N, af=AF_V16)
        _upload(b, tr)

        def run(flags, out):
            eng._check(L.cls_classify_batch(eng.h, t.id, b.h, out.ctypes.data, flags))
            return out

        sentinel = np.full(N, 0xEE, np.uint8)
        b.upload(_abi.BF_VERDICT, sentinel)
        c = run(_abi.F_FORCE_LINEAR, np.zeros(t.n_rules + 1, np.uint64))
        _same(b.download(_abi.BF_VERDICT), ov, "linear verdicts")
        _same(c, oc, "linear counters")

        b.upload(_abi.BF_VERDICT, sentinel)
        c = run(_abi.F_NO_VERDICT, np.zeros(t.n_rules + 1, np.uint64))
        _same(b.download(_abi.BF_VERDICT), sentinel, "untouched verdicts")
        _same(c, oc, "counters without verdicts")
        c = run(_abi.F_NO_VERDICT | _abi.F_FORCE_LINEAR, np.zeros(t.n_rules + 1, np.uint64))
        _same(b.download(_abi.BF_VERDICT), sentinel, "untouched verdicts (linear)")
        _same(c, oc, "linear counters without verdicts")

        pre = np.arange(t.n_rules + 1, dtype=np.uint64) * np.uint64(1000003) + np.uint64(1 << 40)
        c = run(_abi.F_ACCUMULATE, pre.copy())
        _same(c, pre + oc, "accumulated counters")
        _same(b.download(_abi.BF_VERDICT), ov, "verdicts")
        c = run(0, pre.copy())                                      # without the flag: overwritten
        _same(c, oc, "counters")
    finally:
        eng.close()


# ---- 3, 4: connection batches on shards -----------------------------------

def _install(eng, fam):
    """conn_case(fam)'s ACLs on the engine and a connection batch holding its
    connections."""
    from test_gpu_connect_scale import build
    case = conn_case(fam)
    ifs, bind, by_name, pool, spec = build(eng, seed=CONN_SEED, n_local=CONN_LOCALS, n_if=CONN_IFS, fam=fam)
    assert ifs == case["ifs"] and bind == case["bind"]
    ids = np.array([eng.if_id(x) for x in ifs], np.uint32)
    b = eng.batch(case["n"], af=AF_V16 if fam == 16 else AF_V4, conn=True)
    tr = dict(case["tr"], sif=ids[case["si"]], dif=ids[case["di"]])
    _upload(b, tr, CONN_FIELDS)
    return case, b


def _connect_modes(eng, case, b):
    """auto, classifier (counted) and linear: each mode's verdicts over a
    sentinel; the counters of the one counted call."""
    for mode in ("auto", "classifier", "linear"):
        b.upload(_abi.BF_VERDICT, np.full(case["n"], 0xEE, np.uint8))
        eng.connect_batch_b(b, mode=mode, count=(mode == "classifier"))
        _same(b.download(_abi.BF_VERDICT), case["want"], mode)   # ordered behind the connect on every shard
    for name in case["by_name"]:
        _same(eng.conn_counters(name), case["counts"][name], name)
    assert len(set(case["want"].tolist())) >= 3
    assert sum(int(v.sum()) for v in case["counts"].values()) > case["n"] // 4


@pytest.mark.parametrize("pair16", [1, 0])
def test_connect16_on_four_shards(pair16, libopt, capfd):
    """A 16-byte connection batch over four shards: every shard's engine
    evaluates its large ACLs with classify16_pair (conn_pair16=1) or the two
    slot launches (0), as the options set on the primary say -- debug_conn
    makes every engine that has the option print its launches, so four
    engines print -- and the verdicts and the counters summed over the shards
    equal orc_test_connection_hits'."""
    eng = Engine(devices=[0] * 4)
    try:
        libopt.set("conn_pair16", pair16, eng)
        libopt.set("debug_conn", 1, eng)
        case, b = _install(eng, 16)
        sizes = [s[2] for s in b.shards()]
        assert sizes == [c for _, c in shard_starts(case["n"], 4)]
        capfd.readouterr()
        _connect_modes(eng, case, b)
    finally:
        eng.close()
    err = capfd.readouterr().err.splitlines()
    launches = sorted(int(ln.split()[2]) for ln in err if ln.startswith("connect: n "))
    assert launches == sorted(3 * sizes), launches               # three modes on each of the four engines
    pair = [ln for ln in err if ln.startswith("pair16:")]
    slots = [ln for ln in err if ln.startswith("slots16:")]
    if pair16:
        assert len(pair) >= 4 and not slots, (len(pair), len(slots))
    else:
        assert len(slots) >= 4 and not pair, (len(pair), len(slots))


@pytest.mark.parametrize("fam", [16, 4])
def test_rebind_clears_every_shards_counters(fam):
    """Equal rules put again (acl_put_locked's rebind path: the table stays,
    conn_epoch moves) start the ACL's counters from zero on every shard
    (sync_peers): all zero after the put, and the oracle's counts once, not
    twice, after another counted batch."""
    eng = Engine(devices=[0] * 4)
    try:
        case, b = _install(eng, fam)
        eng.connect_batch_b(b, mode="classifier", count=True)
        _same(b.download(_abi.BF_VERDICT), case["want"], "verdicts")
        for name in case["by_name"]:
            _same(eng.conn_counters(name), case["counts"][name], name)
        # counted on the peers too: no single shard holds the whole count
        assert case["counts"]["global"].sum() > 0
        compiles, rebinds = eng.acl_stats()
        put = []
        for name, rules in case["by_name"].items():
            ing, eg = bound_interfaces(case, name)
            if ing or eg:
                assert eng.acl_put(name, rules, ing, eg) == 0
                put.append(name)
        assert "global" in put and eng.acl_stats() == (compiles, rebinds + len(put))
        for name in put:
            assert not eng.conn_counters(name).any(), name
        eng.connect_batch_b(b, mode="classifier", count=True)
        _same(b.download(_abi.BF_VERDICT), case["want"], "verdicts after the rebind")
        for name in put:
            _same(eng.conn_counters(name), case["counts"][name], name)
    finally:
        eng.close()


# ---- 5: shard edges -------------------------------------------------------

@pytest.mark.parametrize("kind", [8, "comm1"])
@pytest.mark.parametrize("af", [AF_V16, AF_V4])
def test_shard_edges(af, kind):
    """n = 0, 1, 3, 5, 7, 9 over eight shards: empty shards (n < G), shards
    of one or two packets (no vector body), n = 0 -- shards() equals
    cls_shard_range, upload / classify / download equal the oracle, the
    counters sum to n; the same n on the group-of-one communicator."""
    rules, pool = table16()
    G = _n_shards(kind)
    eng = _engine(kind)
    try:
        t = eng.put_table("t", rules)
        for n in EDGE_NS:
            tr = batch16(n, 40 + n) if af == AF_V16 else batch4(n, 40 + n, pool)
            ov, oc = classify_ref(rules, tr, 16 if af == AF_V16 else 4)
            b = eng.batch(n, af=af)
            sh = b.shards()
            assert [(s[1], s[2]) for s in sh] == [shard_range(n, G, g) for g in range(G)] == shard_starts(n, G), n
            if G == 8:
                assert sum(s[2] == 0 for s in sh) == max(0, 8 - n), n       # empty shards
                assert all(s[2] < 4 for s in sh), n                          # no vector body anywhere
            _upload(b, tr)
            c = eng.classify_batch(t, b)
            _same(b.download(_abi.BF_VERDICT), ov, "verdicts, n = %d" % n)
            _same(c, oc, "counters, n = %d" % n)
            assert int(c.sum()) == n
            for f, k in INPUTS:
                _same(b.download(f), tr[k], "%s, n = %d" % (k, n))
            # enqueued only; read later
            assert eng.classify_batch(t, b, counters=False) is None
            b.wait()
            _same(b.counters(t.n_rules), oc, "counters read later, n = %d" % n)
            b.close()
    finally:
        eng.close()


def test_empty_batch_every_call_ok():
    """n = 0: every batch call returns CLS_OK (the generators, a connection
    batch and the mirror included) and the counters are all zero."""
    L = _abi.lib()
    rules, _ = table16()
    for kind in (8, "comm1"):
        eng = _engine(kind)
        try:
            t = eng.put_table("t", rules)
            for af, cfg in ((AF_V16, 5), (AF_V4, 3)):
                b = eng.batch(0, af=af, conn=True, mirror=True)
                assert all(s[1:] == (0, 0) for s in b.shards())
                b.gen_traffic(workload.config(cfg)[1], 777)
                for f in FIELDS16:
                    b.upload(f)                                   # the mirror
                    b.download(f, mirror=True)
                    assert len(b.download(f)) == 0
                c = np.full(t.n_rules + 1, 7, np.uint64)
                assert L.cls_classify_batch(eng.h, t.id, b.h, c.ctypes.data, 0) == _abi.OK
                assert not c.any()
                eng.connect_batch_b(b, count=True)
                b.wait()
                assert not b.counters(t.n_rules).any()
                b.close()
        finally:
            eng.close()


# ---- 6: windows -----------------------------------------------------------

def _window_reads(n, G):
    st = [a for a, _ in shard_starts(n, G)]
    return [(0, n), (1, 5), (st[1] - 3, 7), (st[1], 1), (st[1] - 1, st[2] - st[1] + 2), (n - 9, 9), (n, 0)]


@pytest.mark.parametrize("mirror", [False, True])
def test_windows_against_model(mirror):
    """Window writes and reads of a 16-byte connection batch over three
    shards against a numpy model: batch_move's lo / hi clipping, the device
    offset (lo - s.first) * eb and the host offset (lo - first) * eb (the
    mirror: lo * eb) at element widths 16, 2, 1 and 4."""
    G, n = 3, N
    rng = np.random.default_rng(66)
    model = BatchModel(n, FIELDS16)
    wins = windows(n, G)
    assert [crosses(a, k, n, G) for a, k in wins] == [0, 1, 1, 2, 0, 0] and wins[0][0] % 2
    eng = Engine(devices=[0] * G)
    try:
        b = eng.batch(n, af=AF_V16, conn=True, mirror=mirror)
        assert [(s[1], s[2]) for s in b.shards()] == shard_starts(n, G)
        for f, eb in FIELDS16.items():
            whole = random_field(rng, n, eb)
            b.upload(f, whole)
            model.write(f, 0, whole)
            if mirror:
                b.mirror(f)[:] = 0xA5
            for first, k in wins:
                data = random_field(rng, k, eb)
                model.write(f, first, data)
                if mirror:                   # from the mirror at first != 0 ...
                    m = b.mirror(f)
                    m[first:first + k] = data
                    b.upload(f, None, first, k)
                    m[first:first + k] = 0xA5
                else:
                    b.upload(f, data, first, k)
                for a, c in _window_reads(n, G):
                    what = "field %d write %d+%d read %d+%d" % (f, first, k, a, c)
                    _same(b.download(f, a, c), model.read(f, a, c), what)
                    if mirror and c < n:     # ... and into it: the window, and nothing around it
                        b.download(f, a, c, mirror=True)
                        m = b.mirror(f)
                        _same(m[a:a + c], model.read(f, a, c), "mirror, field %d read %d+%d" % (f, a, c))
                        assert (m[:a] == 0xA5).all() and (m[a + c:] == 0xA5).all(), (f, a, c)
                        m[a:a + c] = 0xA5
    finally:
        eng.close()


def test_window_refusals():
    """What batch_move refuses, each with its message; the batch is unchanged."""
    L = _abi.lib()
    n = 1000
    eng = Engine(devices=[0] * 3)
    try:
        plain = eng.batch(n, af=AF_V16)
        conn = eng.batch(n, af=AF_V16, conn=True, mirror=True)
        src = np.arange(n, dtype=np.uint16)
        plain.upload(_abi.BF_DPORT, src)
        buf = np.zeros(2 * n, np.uint16)
        out = "packets out of the batch"
        for b, f, first, k, host, msg in (
                (plain, _abi.BF_DPORT, n + 1, 0, buf, out),                       # first > n
                (plain, _abi.BF_DPORT, 1, n, buf, out),                           # first + n > n
                (plain, _abi.BF_DPORT, n, 1, buf, out),
                (plain, _abi.BF_DPORT, (1 << 64) - 1, 2, buf, out),               # first + n wraps
                (plain, _abi.BF_DPORT, 2, (1 << 64) - 1, buf, out),
                (plain, _abi.BF_SRC_IF, 0, n, buf, "batch has no field 6"),       # not a connection batch
                (plain, _abi.BF_DST_IF, 0, n, buf, "batch has no field 7"),
                (conn, 8, 0, n, buf, "batch has no field 8"),                     # CLS_BF_COUNT
                (conn, 0xFFFFFFFF, 0, n, buf, "batch has no field 4294967295"),
                (plain, _abi.BF_DPORT, 0, n, None, "no host pointer and no mirror (CLS_BATCH_MIRROR)")):
            p = None if host is None else host.ctypes.data
            for call in (L.cls_batch_upload, L.cls_batch_download):
                assert call(b.h, f, first, k, p) == _abi.E_INVAL, (call.__name__, f, first, k)
                assert _last_error(eng) == msg, (call.__name__, f, first, k)
        assert not buf.any()
        _same(plain.download(_abi.BF_DPORT), src, "unchanged")
        conn.upload(_abi.BF_SRC_IF)                                 # a connection batch with a mirror takes both
        conn.download(_abi.BF_SRC_IF, mirror=True)
    finally:
        eng.close()


# ---- 7: chunked staging ---------------------------------------------------

def test_three_staging_chunks():
    """64 MiB + 80 B of addresses from pageable memory on one device: three
    staging chunks up (buffer 0 reused for the third) and down (prev_o /
    prev_m unpack chunk c - 1 while chunk c copies), and a window that starts
    inside the first chunk and needs two of its own."""
    n = N_CHUNKED
    assert stage_chunks(16 * n) == 3 and 16 * n > 2 * STAGE_BYTES
    rng = np.random.default_rng(7)
    data = np.frombuffer(rng.bytes(16 * n), np.uint8).reshape(n, 16)
    first, k = (1 << 20) + 3, (2 << 20) + 1000
    per = STAGE_BYTES // 16                                     # elements a chunk
    assert first % per and first // per != (first + k) // per and stage_chunks(16 * k) == 2
    eng = Engine(0)
    try:
        b = eng.batch(n, af=AF_V16)
        b.upload(_abi.BF_SRC, data)
        assert np.array_equal(b.download(_abi.BF_SRC), data)
        assert np.array_equal(b.download(_abi.BF_SRC, first, k), data[first:first + k])
    finally:
        eng.close()


# ---- 8: two tables on one batch -------------------------------------------

@pytest.mark.parametrize("kind", ["comm1", 2])
@pytest.mark.parametrize("af", [AF_V4, AF_V16])
def test_two_tables_on_one_batch(af, kind):
    """Tables of 50 and 400 rules on one batch: small, small, large, small,
    large, large -- the third call grows counter buffer 0 and the sixth
    buffer 1, each after a smaller all-reduce on it (group of one: rec_red
    set; two shards: summed on the host) -- every call's counters equal its
    oracle's; then the refusals of cls_batch_counters and of a foreign
    batch."""
    L = _abi.lib()
    small, big, tr, (sv, sc), (bv, bc) = two_tables(af)
    eng = _engine(kind)
    other = Engine(0)
    try:
        ts, tb = eng.put_table("small", small), eng.put_table("big", big)
        assert tb.n_rules + 1 > ts.n_rules + 1 == 51                # n_ctr grows
        b = eng.batch(N, af=af)
        # before any classify
        with pytest.raises(ClsError, match="no cls_classify_batch on this batch yet"):
            b.counters(tb.n_rules)
        _upload(b, tr)
        for i, t in enumerate((ts, ts, tb, ts, tb, tb)):
            wv, wc = (sv, sc) if t is ts else (bv, bc)
            _same(eng.classify_batch(t, b), wc, "call %d counters" % i)
            _same(b.download(_abi.BF_VERDICT), wv, "call %d verdicts" % i)
        assert not np.array_equal(sv, bv)
        # enqueued only: small, large, small, then read -- the last call's
        for t in (ts, tb, ts):
            assert eng.classify_batch(t, b, counters=False) is None
        _same(b.counters(ts.n_rules), sc, "the last call's counters")
        wide = np.full(tb.n_rules + 1, 9, np.uint64)               # a longer vector: the first R + 1 entries
        eng._check(L.cls_batch_counters(b.h, wide.ctypes.data, len(wide)))
        _same(wide[:ts.n_rules + 1], sc, "counters into a longer vector")
        assert (wide[ts.n_rules + 1:] == 9).all()
        assert eng.classify_batch(tb, b, counters=False) is None
        short = np.zeros(tb.n_rules, np.uint64)
        assert L.cls_batch_counters(b.h, short.ctypes.data, tb.n_rules) == _abi.E_INVAL
        assert _last_error(eng) == "counters need %u entries" % (tb.n_rules + 1)
        assert not short.any()
        _same(b.counters(tb.n_rules), bc, "after the refusal")
        # a batch of another engine
        to = other.put_table("small", small)
        assert L.cls_classify_batch(other.h, to.id, b.h, None, 0) == _abi.E_INVAL
        assert _last_error(other) == "the batch belongs to another engine"
        assert L.cls_batch_connect(other.h, b.h, 0) == _abi.E_INVAL
        assert _last_error(other) == "the batch belongs to another engine"
    finally:
        eng.close()
        other.close()


# ---- 9: options reach the peers -------------------------------------------

@pytest.mark.parametrize("key,value", [("other_cap", 0), ("other_cap", 1000), ("lds_budget", 256)])
def test_options_reach_the_peers(key, value, libopt):
    """An option set on the primary before the put (other_cap: the OTHER
    queue's size, 30 % protocol 47 to fill it; lds_budget=256: the image in
    global memory) with eight shards: every device engine's table equals the
    primary's (lds_budget: not LDS-resident on any), verdicts and counters
    equal the oracle's in both layouts; a peer refuses options of its own.
    (That the peers hold the primary's Opts shows in
    test_connect16_on_four_shards: the table's form travels with the table.)"""
    rules, pool = table16()
    eng = Engine(devices=[0] * 8)
    try:
        libopt.set(key, value, eng)
        t = eng.put_table("t", rules)
        info = t.info()
        assert info["has_v16"] == 1
        if key == "lds_budget":
            assert info["lds_resident"] == 0 and info["lds_resident_v16"] == 0, info
        for g in range(8):
            assert Table(eng.device_engine(g), t.id, t.n_rules, "t").info() == info, g
        for af in (AF_V16, AF_V4):
            tr = batch16(N, 9, other=0.3) if af == AF_V16 else batch4(N, 9, pool, other=0.3)
            assert 0.25 < (tr["proto"] == 47).mean() < 0.35
            ov, oc = classify_ref(rules, tr, 16 if af == AF_V16 else 4)
            b = eng.batch(N, af=af)
            _upload(b, tr)
            _same(eng.classify_batch(t, b), oc, "counters, af %d" % af)
            _same(b.download(_abi.BF_VERDICT), ov, "verdicts, af %d" % af)
            b.close()
        with pytest.raises(ClsError, match="configure a multi-device engine through its primary engine"):
            eng.device_engine(3).set_option(key, value)
    finally:
        eng.close()


# ---- 10: two distinct devices ---------------------------------------------

def _gpu_count():
    import torch                            # counting devices does not initialise HIP
    return torch.cuda.device_count()


@pytest.mark.skipif(_gpu_count() < 2, reason="needs two GPUs (distinct devices: an RCCL communicator)")
def test_two_distinct_devices_16_byte_batches(single16):
    """Cases 2 and 3 on devices [0, 1]: the 16-byte table uploaded to the
    second GPU (p16's image, d_src_search, d_slot_rule), counters merged by
    the all-reduce over two ranks, a counted 16-byte connection batch."""
    eng = Engine(devices=[0, 1])
    try:
        assert eng.comm_info() == (2, 0)
        _classify16(eng, single16)
        case, b = _install(eng, 16)
        _connect_modes(eng, case, b)
    finally:
        eng.close()
