"""rfx.cache: the one bounded cache of the host code and its lease, and the free list of the exact mode's pinned exchange buffers
(rfx.ops._ExchangePool) -- the two places that decide how long a shared host buffer lives.  No GPU: the free list runs on a plain
numpy allocator and on events whose completion the test sets.  The expected values are written out from the rules: least recently
used first, a hit is a use; a lease holds what any cache returned while it was open; a set is handed out again only after the event
it came back with has completed, and at most 8 idle sets are kept."""
import gc
import threading
import weakref

import numpy as np

from rfx import ops
from rfx.cache import BoundedCache, lease


class Thing:
    """A plain object a weakref can watch."""


def test_bound_hit_moves_to_end_and_oldest_first_eviction():
    c = BoundedCache(3)
    made = []

    def make(k):
        def f():
            made.append(k)
            return "v%s" % k
        return f
    assert len(c) == 0 and "a" not in c
    assert [c.get(k, make(k)) for k in "abc"] == ["va", "vb", "vc"]
    assert len(c) == 3 and all(k in c for k in "abc")
    assert c.get("a", make("a")) == "va"            # a hit: "a" is now the youngest
    assert made == ["a", "b", "c"]                  # make ran once per miss, not on the hit
    c.get("d", make("d"))                           # one over the bound: "b", the oldest, goes
    assert len(c) == 3 and "b" not in c and all(k in c for k in "acd")
    c.get("e", make("e"))                           # then "c"; "a" survived because of its hit
    assert "c" not in c and all(k in c for k in "ade")
    assert c.get("b", make("b")) == "vb"            # evicted: made again
    assert made == ["a", "b", "c", "d", "e", "b"] and "a" not in c
    c.clear()
    assert len(c) == 0 and "d" not in c
    c.get("d", make("d"))
    assert made[-1] == "d"


def test_lease_records_hits_and_misses_and_nests():
    c, d = BoundedCache(4), BoundedCache(4)
    c.get(1, lambda: "one")                         # no lease open: nobody records it
    with lease() as outer:
        assert outer == []
        c.get(1, lambda: "never")                   # a hit
        d.get(2, lambda: "two")                     # a miss, of another cache
        with lease() as inner:
            c.get(3, lambda: "three")
        d.get(2, lambda: "never")
    c.get(4, lambda: "four")                        # closed: no longer recorded
    assert inner == ["three"]
    assert outer == ["one", "two", "three", "two"]


def test_lease_is_per_thread():
    c = BoundedCache(4)
    started, go = threading.Event(), threading.Event()
    theirs = []

    def other():
        c.get("x", lambda: "other thread, no lease")
        with lease() as held:
            started.set()
            go.wait(10)
            c.get("y", lambda: "other thread")
        theirs.extend(held)
    t = threading.Thread(target=other)
    t.start()
    assert started.wait(10)
    with lease() as mine:
        c.get("z", lambda: "main thread")
        go.set()
        t.join(10)
    assert mine == ["main thread"] and theirs == ["other thread"]


def test_an_evicted_value_lives_as_long_as_a_lease_list_holds_it():
    c = BoundedCache(1)
    with lease() as held:
        ref = weakref.ref(c.get("a", Thing))
    loose = weakref.ref(c.get("b", Thing))          # evicts "a"
    c.get("c", Thing)                               # evicts "b", which no lease holds
    gc.collect()
    assert "a" not in c and "b" not in c
    assert loose() is None
    assert ref() is not None and held == [ref()]
    del held
    gc.collect()
    assert ref() is None


# ---------------------------------------------------------------- the exchange-buffer free list


class StubEvent:
    def __init__(self, done=False):
        self.done = done

    def query(self):
        return self.done


def _numpy_pool(monkeypatch):
    monkeypatch.setattr(ops, "_alloc_exchange", lambda n_off, rows: dict(off=np.zeros(n_off, np.int32), xy=np.empty((rows, 16), np.float32),
                                                                        H=np.empty((rows, 9), np.float32)))
    return ops._ExchangePool()


def test_a_set_is_reused_only_after_its_event_has_completed(monkeypatch):
    pool = _numpy_pool(monkeypatch)
    a = pool.take(3, 100)
    assert a["off"].shape == (3,) and a["xy"].shape == (100, 16) and a["H"].shape == (100, 9)
    assert pool.allocations == 1
    ev = StubEvent(done=False)
    pool.give(a, ev)
    b = pool.take(3, 100)                           # the patch kernel of a's last owner may still read a["H"]
    assert b is not a and pool.allocations == 2
    ev.done = True
    c = pool.take(3, 100)
    assert c is a and pool.allocations == 2
    d = pool.take(3, 100)                           # a is out again, b was never given back
    assert d is not a and d is not b and pool.allocations == 3


def test_outstanding_takes_never_share_a_set(monkeypatch):
    pool = _numpy_pool(monkeypatch)
    first = [pool.take(3, 64) for _ in range(4)]
    assert len({id(s) for s in first}) == 4 and pool.allocations == 4
    for s in first:
        pool.give(s, StubEvent(done=True))
    second = [pool.take(3, 64) for _ in range(5)]
    assert len({id(s) for s in second}) == 5 and pool.allocations == 5
    assert {id(s) for s in first} <= {id(s) for s in second}


def test_a_set_too_small_is_passed_over(monkeypatch):
    pool = _numpy_pool(monkeypatch)
    small = pool.take(3, 64)
    pool.give(small, StubEvent(done=True))
    big = pool.take(3, 65)                          # more rows than the idle set has
    assert big is not small and big["xy"].shape[0] == 65 and pool.allocations == 2
    wide = pool.take(4, 64)                         # more offsets than it has
    assert wide is not small and wide["off"].shape[0] == 4 and pool.allocations == 3
    assert pool.take(2, 10) is small and pool.allocations == 3


def test_idle_sets_are_bounded_and_the_oldest_go_first(monkeypatch):
    pool = _numpy_pool(monkeypatch)
    assert pool.MAX_IDLE == 8
    sets = [pool.take(3, 64) for _ in range(11)]
    assert pool.allocations == 11
    for s in sets:
        pool.give(s, StubEvent(done=True))
    assert len(pool.idle) == 8
    again = [pool.take(3, 64) for _ in range(9)]
    assert [id(s) for s in again[:8]] == [id(s) for s in sets[3:]]      # the three given back first were dropped
    assert pool.allocations == 12 and len(pool.idle) == 0


def test_a_set_whose_event_is_pending_is_never_dropped(monkeypatch):
    pool = _numpy_pool(monkeypatch)
    sets = [pool.take(3, 64) for _ in range(10)]
    events = [StubEvent(done=k >= 2) for k in range(10)]       # the two oldest are still read by their patch kernels
    for s, ev in zip(sets, events):
        pool.give(s, ev)
    assert [id(s) for s, _ in pool.idle] == [id(s) for s in sets]       # nothing beyond the bound has completed: all ten stay
    events[1].done = True
    extra = pool.take(3, 64)                                            # sets[1]: the oldest whose event has completed
    assert extra is sets[1]
    pool.give(extra, StubEvent(done=True))
    # ten again, two over the bound: sets[0] is pending and stays, sets[2] has completed and goes
    assert [id(s) for s, _ in pool.idle] == [id(sets[k]) for k in (0, 3, 4, 5, 6, 7, 8, 9, 1)]
    events[0].done = True
    pool.give(pool.take(3, 65), StubEvent(done=True))                   # a new, larger set comes back: sets[0] and sets[3] go
    assert [id(s) for s, _ in pool.idle][:7] == [id(sets[k]) for k in (4, 5, 6, 7, 8, 9, 1)] and len(pool.idle) == 8


def test_concurrent_takers_get_distinct_sets(monkeypatch):
    pool = _numpy_pool(monkeypatch)
    for s in [pool.take(3, 64) for _ in range(8)]:
        pool.give(s, StubEvent(done=True))
    got, barrier = [], threading.Barrier(8)

    def taker():
        barrier.wait(10)
        for _ in range(50):
            s = pool.take(3, 64)
            got.append(id(s))
            pool.give(s, StubEvent(done=True))
    threads = [threading.Thread(target=taker) for _ in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(30)
    assert len(got) == 400 and len(pool.idle) == 8 and len({id(s) for s, _ in pool.idle}) == 8
    assert pool.allocations == 8                    # a set is always idle when a thread asks: none had to be allocated
