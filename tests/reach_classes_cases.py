"""The reachability-classes tests' shared reference and matrices
(tests/test_reach_classes_cpu.py, tests/test_gpu_reach_classes.py).

classes_ref is the definition restated: endpoints s and t are equivalent iff
exchanging them leaves the [P, N, N] matrix unchanged; an endpoint joins the
first class whose representative it is equivalent to (the relation is an
equivalence, so the representative decides), which numbers the classes by
ascending smallest member.  The synthetic matrices are computed once and are
read-only."""
import functools

import numpy as np

NONE = 255

# planted block matrices: (N, P, C)
PLANTED = ((1, 1, 1), (2, 1, 1), (3, 1, 2), (63, 3, 5), (64, 1, 64), (65, 2, 7), (130, 3, 9), (1000, 2, 40),
           (64, 1, 40))
OTHERS = ("bytes", "symmetric", "asym_pair", "diag_pair", "equal", "random")
NAMES = tuple("planted_%d_%d_%d" % k for k in PLANTED) + OTHERS


def twin(m, s, t) -> bool:
    """The definition, literally: the matrix with s and t exchanged is the matrix."""
    perm = np.arange(m.shape[1])
    perm[s], perm[t] = t, s
    return bool((m[:, perm][:, :, perm] == m).all())


def classes_ref(m):
    """(classes [N] u32, reps [C] u32, sizes [C] u32, self [P, C] u8, quot
    [P, C, C] u8) of a [P, N, N] uint8 matrix."""
    m = np.asarray(m)
    P, N, _ = m.shape
    classes = np.zeros(N, np.uint32)
    reps = []
    for s in range(N):
        hit = -1
        if reps:
            R = np.array(reps)
            k = np.arange(len(R))
            rows = m[:, R, :] == m[:, s:s + 1, :]                       # [P, k, d]: M[p, r, d] == M[p, s, d]
            cols = m[:, :, R] == m[:, :, s:s + 1]                       # [P, d, k]: M[p, d, r] == M[p, d, s]
            rows[:, k, R] = True
            rows[:, :, s] = True
            cols[:, R, k] = True
            cols[:, s, :] = True
            ok = rows.all(axis=(0, 2)) & cols.all(axis=(0, 1))
            ok &= (m[:, s, R] == m[:, R, s]).all(axis=0) & (m[:, R, R] == m[:, s, s][:, None]).all(axis=0)
            at = np.flatnonzero(ok)
            if len(at):
                hit = int(at[0])
        if hit < 0:
            hit = len(reps)
            reps.append(s)
        classes[s] = hit
    reps = np.array(reps, np.uint32)
    C = len(reps)
    sizes = np.bincount(classes, minlength=C).astype(np.uint32)
    self_ = np.ascontiguousarray(m[:, reps, reps])
    quot = np.ascontiguousarray(m[:, reps[:, None], reps[None, :]])
    for c in range(C):
        members = np.flatnonzero(classes == c)
        quot[:, c, c] = m[:, members[0], members[1]] if len(members) > 1 else NONE
    if N <= 40:
        for s in range(N):
            for t in range(s + 1, N):
                assert twin(m, s, t) == (classes[s] == classes[t]), (s, t)
    return classes, reps, sizes, self_, quot


def expand(classes, self_, quot):
    """The matrix of a summary (the tests' own restatement of the reconstruction)."""
    c = np.asarray(classes).astype(np.int64)
    N = len(c)
    m = np.empty((quot.shape[0], N, N), np.uint8)
    for s in range(N):
        m[:, s, :] = quot[:, c[s], :][:, c]
        m[:, s, s] = self_[:, c[s]]
    return m


def planted(N, P, C, seed=0, values=(0, 1, 2, 3)):
    """A random class map onto C non-empty classes, random self and quot."""
    rng = np.random.default_rng(7000 + 131 * N + 17 * P + C + seed)
    cls = np.concatenate([np.arange(C), rng.integers(0, C, N - C)])
    rng.shuffle(cls)
    vals = np.array(values, np.uint8)
    quot = vals[rng.integers(0, len(vals), (P, C, C))]
    self_ = vals[rng.integers(0, len(vals), (P, C))]
    return expand(cls, self_, quot)


@functools.lru_cache(maxsize=None)
def synthetic(name):
    """A read-only [P, N, N] uint8 matrix by name (NAMES)."""
    rng = np.random.default_rng(99)
    if name.startswith("planted_"):
        m = planted(*[int(x) for x in name.split("_")[1:]])
    elif name == "bytes":                     # bytes above the ConnectionActions
        m = planted(33, 2, 5, values=(0xA5, 255, 0, 7, 128))
    elif name == "symmetric":                 # 0 / 1, equal to its transpose
        m = planted(48, 1, 6, values=(0, 1))
        m = np.maximum(m, m.transpose(0, 2, 1))
    elif name == "asym_pair":                 # 2 and 4 differ only in M[2, 4] against M[4, 2]
        m = np.ones((1, 6, 6), np.uint8)
        m[0, 2, 4] = 2
    elif name == "diag_pair":                 # 3 differs from the others only on the diagonal
        m = np.ones((1, 5, 5), np.uint8)
        m[0, 3, 3] = 0
    elif name == "equal":
        m = np.full((2, 70, 70), 2, np.uint8)
    elif name == "random":
        m = rng.integers(0, 4, (1, 130, 130)).astype(np.uint8)
    else:
        raise KeyError(name)
    m = np.ascontiguousarray(m, np.uint8)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def synthetic_ref(name):
    return classes_ref(synthetic(name))


@functools.lru_cache(maxsize=None)
def oracle_ref(fam):
    """classes_ref of the oracle's matrix of reach_cases.case(fam)."""
    import reach_cases as rc
    return classes_ref(rc.case(fam)["want"])
