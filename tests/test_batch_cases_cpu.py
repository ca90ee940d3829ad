"""The arithmetic tests/test_gpu_batches.py relies on, without a GPU: the
shard starts of every (n, G) it uses against cls_shard_range, the staging
chunk counts, which windows cross which boundaries, and that its tables have
16-byte classifiers (cls_compile_v16)."""
import numpy as np
import pytest

from vpp_amd import _abi
from batch_cases import (EDGE_NS, FIELDS16, N, N_CHUNKED, STAGE_BYTES, BatchModel, batch16, crosses, random_field,
                         shard_starts, stage_chunks, table16, two_tables, windows)
from cls_image import compile_blob
from vpp_amd.engine import shard_range


@pytest.mark.parametrize("n,G", [(N, G) for G in (1, 2, 3, 4, 5, 7, 8)] + [(n, 8) for n in EDGE_NS] +
                         [(20003, 4), (N_CHUNKED, 1)])
def test_shard_starts_are_the_librarys(n, G):
    st = shard_starts(n, G)
    assert st == [shard_range(n, G, g) for g in range(G)]
    assert st[0][0] == 0 and sum(c for _, c in st) == n
    assert all(a + c == b for (a, c), (b, _) in zip(st, st[1:]))


def test_sizes_reach_their_branches():
    # ragged shards whose starts are no multiples of 4 and whose tails are no whole vector groups
    for G in (3, 8):
        st = shard_starts(N, G)
        assert any(a % 4 for a, _ in st) and any(c % 4 for _, c in st) and len({c for _, c in st}) == 2
    assert all(a % 4 for a, _ in shard_starts(N, 3)[1:])
    # eight shards of at most 9 packets: empty ones below 8, none with a vector body
    for n in EDGE_NS:
        st = shard_starts(n, 8)
        assert sum(c == 0 for _, c in st) == max(0, 8 - n) and all(c < 4 for _, c in st)
    # three staging chunks, the third in buffer 0 again (chunk c uses buffer c & 1)
    assert stage_chunks(16 * N_CHUNKED) == 3 == -(-16 * N_CHUNKED // (1 << 25)) and STAGE_BYTES == 32 << 20
    assert stage_chunks(16 * N_CHUNKED - 96) == 2            # ... by 80 bytes
    # the existing round trip's shards move one chunk each
    assert stage_chunks(4 * shard_starts((9 << 20) + 3, 2)[1][1]) == 1
    # the windows: inside shard 0, across each boundary, across both, empty at both ends
    w = windows(N, 3)
    assert [crosses(a, k, N, 3) for a, k in w] == [0, 1, 1, 2, 0, 0]
    assert w[-2:] == [(0, 0), (N, 0)] and w[0][0] % 2 == 1 and all(a + k <= N for a, k in w)


def test_model_window_writes():
    rng = np.random.default_rng(1)
    m = BatchModel(100, FIELDS16)
    for f, eb in FIELDS16.items():
        whole = random_field(rng, 100, eb)
        m.write(f, 0, whole)
        part = random_field(rng, 7, eb)
        m.write(f, 31, part)
        want = whole.copy()
        want[31:38] = part
        assert np.array_equal(m.read(f), want) and np.array_equal(m.read(f, 30, 3), want[30:33])
        assert m.read(f).itemsize * (16 if eb == 16 else 1) == eb and len(m.read(f, 100, 0)) == 0


def test_tables_have_16_byte_classifiers():
    small, big, tr, _, _ = two_tables(16)
    for rules in (table16()[0], small, big):
        assert len(compile_blob(_abi.CRules(rules), "cls_compile_v16")) > 0
    assert len(small) == 50 and len(big) == 400
    tr = batch16(1000, 3)
    assert (tr["proto"][-3:] == 47).all() and tr["src"].shape == (1000, 16)
    twins = (tr["src"][:, :4] == (0xFD, 0, 0, 0x30)).all(1)
    assert 0.3 < twins.mean() < 0.7                          # the rest IPv4-mapped
