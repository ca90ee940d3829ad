"""Cases of tests/test_gpu_batches.py: the sizes, a numpy model of an
engine-owned batch, and the shared inputs with their oracle results.

Nothing here touches a device.  The arithmetic the GPU tests rely on (shard
starts, staging chunks) is restated in plain Python and checked against the
library's cls_shard_range in tests/test_batch_cases_cpu.py.
"""
import functools

import numpy as np

import oracle
from aclgen import mix_families, random_acl, random_acl16, random_traffic
from vpp_amd import _abi

# ragged: three shards of 65539 / 65540 / 65540, eight of 24577 or 24578;
# no shard start but 0 is a multiple of 4 at G = 3
N = 3 * (1 << 16) + 11
STAGE_BYTES = 1 << 25                    # fleet.cpp kStageBytes
N_CHUNKED = (4 << 20) + 5                # 16-byte addresses: 64 MiB + 80 B
EDGE_NS = (0, 1, 3, 5, 7, 9)             # over eight shards: empty and tail-only shards

# field -> element bytes (16-byte layout; the IPv4 layout has 4-byte addresses)
FIELDS16 = {_abi.BF_SRC: 16, _abi.BF_DST: 16, _abi.BF_SPORT: 2, _abi.BF_DPORT: 2, _abi.BF_PROTO: 1,
            _abi.BF_VERDICT: 1, _abi.BF_SRC_IF: 4, _abi.BF_DST_IF: 4}
INPUTS = ((_abi.BF_SRC, "src"), (_abi.BF_DST, "dst"), (_abi.BF_SPORT, "sport"), (_abi.BF_DPORT, "dport"),
          (_abi.BF_PROTO, "proto"))


def shard_starts(n: int, G: int):
    """[(first, count)] of the G shards of n packets: [g n / G, (g + 1) n / G)."""
    return [(g * n // G, (g + 1) * n // G - g * n // G) for g in range(G)]


def stage_chunks(n_bytes: int) -> int:
    """Staging chunks a pageable transfer of n_bytes takes (move_piece)."""
    return -(-n_bytes // STAGE_BYTES)


def windows(n: int, G: int):
    """(first, count) window writes over G shards of n packets: inside shard
    0 at an odd start, one element on each side of every boundary, all the
    shards at once, and empty windows at both ends."""
    st = [a for a, _ in shard_starts(n, G)]
    out = [(1001, 777)]
    out += [(a - 1, 2) for a in st[1:]]
    out += [(st[1] - 5, st[-1] + 7 - (st[1] - 5)), (0, 0), (n, 0)]
    return out


def crosses(first: int, count: int, n: int, G: int) -> int:
    """Shard boundaries strictly inside [first, first + count)."""
    return sum(first < a < first + count for a, _ in shard_starts(n, G)[1:])


def elem_dtype(eb: int):
    return {1: np.uint8, 2: np.uint16, 4: np.uint32, 16: np.uint8}[eb]


def random_field(rng, n: int, eb: int) -> np.ndarray:
    """n random elements of eb bytes in the shape Batch.upload takes."""
    raw = np.frombuffer(rng.bytes(n * eb), np.uint8)
    return raw.reshape(n, 16).copy() if eb == 16 else raw.view(elem_dtype(eb)).copy()


class BatchModel:
    """What a batch holds, field by field, after a sequence of window writes."""

    def __init__(self, n: int, fields: dict):
        self.n, self.fields = n, dict(fields)
        self.a = {f: (np.zeros((n, 16), np.uint8) if eb == 16 else np.zeros(n, elem_dtype(eb)))
                  for f, eb in fields.items()}

    def write(self, f: int, first: int, data: np.ndarray):
        assert 0 <= first and first + len(data) <= self.n
        self.a[f][first:first + len(data)] = data

    def read(self, f: int, first: int = 0, count=None) -> np.ndarray:
        count = self.n - first if count is None else count
        return self.a[f][first:first + count]


# ---- a 16-byte table and batch (case 2) -----------------------------------

@functools.lru_cache(None)
def table16(n_rules: int = 300):
    """(rules, prefix pool): random_acl16's rules, about half of their plain
    IPv4 networks restated as fd00:30::/96 twins (mix_families), so that the
    twins of the batch below meet rules of their own family."""
    rules, pool = random_acl16(5, n_rules, 0.05)
    tiny = random_traffic(1, 4, pool)
    return mix_families(rules, tiny, 7)[0], pool


def batch16(n: int, seed: int, other: float = 0.05, n_rules: int = 300):
    """n 16-byte packets aimed at table16's prefixes: IPv4-mapped or twin
    addresses, `other` of them protocol 47, the last three included."""
    _, pool = table16(n_rules)
    _, tr = mix_families([], random_traffic(seed, n, pool), seed)
    if n:
        rng = np.random.default_rng(seed + 1000)
        o = rng.random(n) < other
        o[-3:] = True
        tr["proto"] = np.where(o, 47, tr["proto"]).astype(np.uint8)
    return tr


def batch4(n: int, seed: int, pool, other: float = 0.05):
    tr = random_traffic(seed, n, pool)
    if n:
        rng = np.random.default_rng(seed + 1000)
        o = rng.random(n) < other
        o[-3:] = True
        tr["proto"] = np.where(o, 47, tr["proto"]).astype(np.uint8)
    return tr


def classify_ref(rules, tr, af: int):
    """The oracle's verdicts and per-rule counters (an empty batch: no
    verdicts, every counter zero)."""
    if len(tr["dport"]) == 0:
        return np.zeros(0, np.uint8), np.zeros(len(rules) + 1, np.uint64)
    return oracle.classify_fast(oracle.rules_to_c(rules), tr["src"], tr["dst"], tr["dport"], tr["proto"], af=af)


@functools.lru_cache(None)
def case16(n: int = N, seed: int = 5):
    """(rules, batch, oracle verdicts, oracle counters), computed once."""
    rules, _ = table16()
    tr = batch16(n, seed)
    v, c = classify_ref(rules, tr, 16)
    for a in list(tr.values()) + [v, c]:
        a.setflags(write=False)
    return rules, tr, v, c


@functools.lru_cache(None)
def two_tables(af: int):
    """Tables of R = 50 and R = 400, a batch of N packets aimed at the larger
    one's prefixes and each table's oracle result (case 8)."""
    gen = random_acl16 if af == 16 else random_acl
    big, pool = gen(400, 400, 0.05)
    small = gen(50, 50, 0.05)[0]
    if af == 16:
        _, tr = mix_families([], random_traffic(8, N, pool), 8)
    else:
        tr = random_traffic(8, N, pool)
    return small, big, tr, classify_ref(small, tr, af), classify_ref(big, tr, af)


# ---- connection batches (cases 3, 4, 10) ----------------------------------

class _Recorder:
    """test_gpu_connect_scale.build's engine when only the ACLs are wanted."""

    def acl_put(self, *_a):
        return 0


CONN_N, CONN_SEED, CONN_LOCALS, CONN_IFS = 20003, 3, 24, 40


@functools.lru_cache(None)
def conn_case(fam: int):
    """The ACLs of build(seed 3, 24 local ACLs, 40 interfaces), 20003
    connections (5 % protocol 47, a tenth from an interface to itself) and
    orc_test_connection_hits' verdicts and per-(ACL, rule) counters."""
    from test_gpu_connect_scale import build, oracle_connections, traffic
    ifs, bind, by_name, pool, spec = build(_Recorder(), seed=CONN_SEED, n_local=CONN_LOCALS, n_if=CONN_IFS, fam=fam)
    n = CONN_N
    rng = np.random.default_rng(9)
    tr = traffic(CONN_SEED, n, pool, spec, fam)
    o = rng.random(n) < 0.05
    o[-3:] = True
    tr["proto"] = np.where(o, 47, tr["proto"]).astype(np.uint8)
    si = rng.integers(0, len(ifs), n).astype(np.uint32)
    di = np.where(rng.random(n) < 0.1, si, rng.integers(0, len(ifs), n)).astype(np.uint32)
    want, counts = oracle_connections(bind, by_name, ifs, si, di, tr, fam)
    return dict(ifs=ifs, bind=bind, by_name=by_name, tr=tr, si=si, di=di, want=want, counts=counts, n=n)


def bound_interfaces(case, name):
    """(ingress, egress) interface names an ACL is still bound to (a later
    ACL of build() may have taken an interface over)."""
    ing = [i for i in case["ifs"] if case["bind"][i][0] == name]
    eg = [i for i in case["ifs"] if case["bind"][i][1] == name]
    return ing, eg
