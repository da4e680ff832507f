"""The one bounded cache of the host code, and the lease that ties what a cache handed out to a longer-lived user.

``BoundedCache`` keeps the most recently used ``max_entries`` values and forgets the oldest first.  A cache only holds its values
while they are young: whoever must outlive an eviction -- a captured HIP graph that baked a cached tensor's address into its
kernels -- opens a ``lease()`` around the calls that read the caches and keeps the list it yields.  Pure Python: no device."""
import collections
import contextlib
import threading

_open = threading.local()       # .lists: the lease lists open in this thread, outermost first


class BoundedCache:
    """Not locked: the host code calls a cache from one thread at a time (leases are per thread all the same)."""

    def __init__(self, max_entries):
        self.max_entries = max_entries
        self._d = collections.OrderedDict()

    def get(self, key, make):
        """The value of ``key``: the cached one (which becomes the most recently used) or ``make()``, stored; more than
        ``max_entries`` values: the least recently used go.  Every lease open in this thread receives the value."""
        if key in self._d:
            self._d.move_to_end(key)
        else:
            self._d[key] = make()
            while len(self._d) > self.max_entries:
                self._d.popitem(last=False)
        v = self._d[key]
        for held in getattr(_open, "lists", ()):
            held.append(v)
        return v

    def clear(self):
        self._d.clear()

    def __len__(self):
        return len(self._d)

    def __contains__(self, key):
        return key in self._d


@contextlib.contextmanager
def lease():
    """Yields a list that receives every value any BoundedCache.get returns in this thread while the block is open, hits and misses
    alike (nested blocks each receive it).  The values live as long as the list does, whatever the caches evict meanwhile."""
    held = []
    lists = _open.__dict__.setdefault("lists", [])
    lists.append(held)
    try:
        yield held
    finally:
        lists.pop()
