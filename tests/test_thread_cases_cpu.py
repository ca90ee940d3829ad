"""The threaded tests' runner and checkers (tests/thread_cases.py) on fakes:
no GPU, no library.

The checkers must reject what a racing engine can produce: a fake engine
updates a two-part state with a sleep between the halves while readers copy it
unlocked, and ``one_of`` has to reject some copy; once the fake takes a lock,
none.  ``run_threads`` has to re-raise a thread's exception, and on a missed
deadline end the pytest session with a non-zero status and a stack dump (run
in a child pytest, since it ends the session it runs in).

Scenario 6's precondition is asserted here on the oracle alone: the two states
the writer toggles between differ in at least 5 % of the matrix's cells, so a
reader that mixed them could not pass for either.
"""
import os
import subprocess
import sys
import textwrap
import threading
import time

import numpy as np
import pytest

import thread_cases as tc

STATES = (np.zeros((2, 64), np.uint8), np.ones((2, 64), np.uint8))


class FakeEngine:
    """A two-part state written half by half; ``lock`` None: readers may see
    one half of each state."""

    def __init__(self, locked):
        self.state = STATES[0].copy()
        self.lock = threading.Lock() if locked else None
        self.done = False

    def put(self, k):
        if self.lock:
            with self.lock:
                self._put(k)
        else:
            self._put(k)

    def _put(self, k):
        self.state[0] = STATES[k][0]
        time.sleep(0.002)
        self.state[1] = STATES[k][1]

    def read(self):
        if self.lock:
            with self.lock:
                return self.state.copy()
        return self.state.copy()


def _toggle(fake, rounds=30):
    """One writer, three readers; the readers' copies."""
    def writer():
        for i in range(rounds):
            fake.put((i + 1) & 1)
            time.sleep(0.002)                  # lets a reader take the lock
        fake.done = True

    def reader():
        seen = []
        while not fake.done:
            seen.append(fake.read())
            time.sleep(0.0005)
        return seen
    res = tc.run_threads([writer] + [reader] * 3, deadline_s=30)
    return [a for seen in res[1:] for a in seen]


def test_one_of_rejects_the_unlocked_fake():
    seen = _toggle(FakeEngine(locked=False))
    assert len(seen) > 30
    bad = 0
    for a in seen:
        try:
            tc.one_of(a, STATES)
        except AssertionError:
            bad += 1
    assert bad > 0, "no torn copy among %d reads of a fake that sleeps between its halves" % len(seen)


def test_one_of_accepts_the_locked_fake():
    seen = _toggle(FakeEngine(locked=True))
    assert len(seen) >= 10
    kinds = {tc.one_of(a, STATES) for a in seen}
    assert kinds <= {0, 1}


def test_one_of_cases():
    a, b = STATES
    assert tc.one_of(a.copy(), [a, b]) == 0 and tc.one_of(b.copy(), [a, b]) == 1
    mixed = a.copy()
    mixed[1, 63] = 1                                   # one cell of the other state
    with pytest.raises(AssertionError, match="no candidate"):
        tc.one_of(mixed, [a, b])
    with pytest.raises(AssertionError, match="not distinct"):
        tc.one_of(a.copy(), [a, a])
    with pytest.raises(AssertionError, match="no candidate"):
        tc.one_of(a[:1], [a, b])                       # another shape equals nothing


def test_sums_to():
    parts = [np.array([1, 2, 3], np.uint64), np.array([10, 0, 2 ** 40], np.uint64)]
    tc.sums_to(np.array([11, 2, 3 + 2 ** 40], np.uint64), parts)
    with pytest.raises(AssertionError, match="sum differs"):
        tc.sums_to(np.array([11, 2, 4 + 2 ** 40], np.uint64), parts)
    with pytest.raises(AssertionError):
        tc.sums_to(np.array([11, 2], np.uint64), parts)


def test_run_threads_returns_results_in_order():
    assert tc.run_threads([lambda i=i: i * i for i in range(tc.T)], deadline_s=30) == [i * i for i in range(tc.T)]


def test_run_threads_reraises_a_threads_exception():
    def boom():
        raise KeyError("from a thread")
    with pytest.raises(KeyError, match="from a thread"):
        tc.run_threads([lambda: 1, boom, lambda: 2], deadline_s=30)


CHILD = """
    import sys
    import threading
    sys.path.insert(0, %r)
    import thread_cases as tc


    class Eng:
        h = 1


    ENG = Eng()


    def test_stuck(capfd):
        tc.run_threads([lambda: None, threading.Event().wait], deadline_s=1.0, engines=[ENG], capture=capfd)


    def test_never_runs():
        raise SystemExit("a test ran after the hang")
"""


def test_deadline_ends_the_session(tmp_path):
    """A thread blocked for ever: the child session ends with status 3 within
    the deadline plus 10 s, the stacks on stderr, and runs no further test."""
    f = tmp_path / "test_child_hang.py"
    f.write_text(textwrap.dedent(CHILD % os.path.dirname(os.path.abspath(__file__))))
    t0 = time.monotonic()
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "--rootdir", str(tmp_path),
                        str(f)], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    took = time.monotonic() - t0
    assert p.returncode == tc.EXIT_HANG, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert took < 1.0 + 10.0, took
    assert "still running after" in p.stderr and "caller1" in p.stderr
    assert "Thread 0x" in p.stderr and "wait" in p.stderr          # faulthandler's dump of the stuck thread
    assert "a test ran after the hang" not in p.stdout + p.stderr
    assert "stuck in a library call" in p.stdout + p.stderr


def test_hang_takes_the_engines_handles():
    """_hang clears the handles before it ends the session."""
    class Eng:
        h = 1
    e = Eng()
    with pytest.raises(pytest.exit.Exception) as ei:
        tc._hang([e], 1.0, ["caller0"])
    assert e.h is None and ei.value.returncode == tc.EXIT_HANG


@pytest.mark.parametrize("fam", [4, 16])
def test_churn_states_differ_enough(fam):
    """Scenario 6's precondition: want0 and want1 differ in >= 5 % of the
    cells, and R1 is R0 behind a leading deny-any rule."""
    c = tc.churn_case(fam)
    assert c["r1"][1:] == c["r0"] and c["r1"][0] == tc.deny_any()
    assert c["ing"] or c["eg"]
    share = tc.differing_share(c["want0"], c["want1"])
    print("churn_case(%d): %s, %.1f %% of %d cells differ" % (fam, c["name"], 100 * share, c["want0"].size))
    assert share >= 0.05
    big = tc.differing_share(c["big0"], c["big1"])
    print("twelve probes: %.1f %% of %d cells differ" % (100 * big, c["big0"].size))
    assert big >= 0.05
    # the matrix readers' call is at least 17 tiles under the smallest tile the library makes
    assert tc.lib_reach_tile(256) == 1024 and tc.tiles(c["big0"].size, 256) >= 17
    assert tc.tiles(c["want0"].size, 256) == 5


def test_hang_takes_batches_and_views_too():
    class Obj:
        def __init__(self):
            self.h, self._batches, self._views = 1, [], []
    e, v, b1, b2 = Obj(), Obj(), Obj(), Obj()
    e._batches, e._views, v._batches = [b1], [v], [b2]
    with pytest.raises(pytest.exit.Exception):
        tc._hang([e], 1.0, ["caller0"])
    assert [x.h for x in (e, v, b1, b2)] == [None] * 4
