"""A minimal list-backed stand-in for ``sortedcontainers.SortedList`` -- the handful of operations the reference's PriorityStore
uses (``add``, ``pop``, ``remove``, indexing / slicing, iteration, ``len``) -- for machines where the package is not installed.
Test code of this repository."""

from __future__ import annotations

import bisect
import sys
import types


class SortedList:
    def __init__(self, iterable=None, key=None):
        self._key = key if key is not None else (lambda x: x)
        self._items: list = []
        for x in iterable or ():
            self.add(x)

    def add(self, value) -> None:
        keys = [self._key(x) for x in self._items]
        self._items.insert(bisect.bisect_right(keys, self._key(value)), value)

    def pop(self, index: int = -1):
        return self._items.pop(index)

    def remove(self, value) -> None:
        for i, x in enumerate(self._items):
            if x is value:
                del self._items[i]
                return
        raise ValueError("value not in list")

    def __getitem__(self, index):
        return self._items[index]

    def __iter__(self):
        return iter(self._items)

    def __len__(self) -> int:
        return len(self._items)


def sorted_list_class():
    """The real SortedList where it is installed, else the stand-in (also injected as ``sortedcontainers`` into sys.modules)."""
    try:
        from sortedcontainers import SortedList as real
        return real
    except ImportError:
        mod = types.ModuleType("sortedcontainers")
        mod.SortedList = SortedList
        sys.modules["sortedcontainers"] = mod
        return SortedList
