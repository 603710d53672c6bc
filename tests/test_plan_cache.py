"""PlanCache (glsdet_amd/plans.py), the LRU cache of compiled plans behind HipDetector.compile and HipGflDetector.compile,
on a counting fake builder: no GPU, no torch."""
import os
import subprocess
import sys
import threading

from glsdet_amd.plans import PlanCache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Builder:
    """build(key) -> a fresh object per call; .calls lists the keys built, in order"""

    def __init__(self):
        self.calls = []

    def __call__(self, key):
        return lambda: (self.calls.append(key), object())[1]


def _fill(cache, build, keys):
    return [cache.get(k, build(k)) for k in keys]


def test_a_hit_returns_the_same_object_and_builds_nothing():
    cache, build = PlanCache(), Builder()
    first = cache.get("a", build("a"))
    assert cache.get("a", build("a")) is first and cache.get("a", build("a")) is first
    assert build.calls == ["a"] and list(cache.entries) == ["a"]


def test_cap_of_two_evicts_the_oldest(monkeypatch):
    monkeypatch.setenv("GLSDET_MAX_PLANS", "2")
    cache, build = PlanCache(), Builder()
    a, b, c = _fill(cache, build, "abc")
    assert list(cache.entries) == ["b", "c"] and cache.entries["b"] is b and cache.entries["c"] is c
    assert cache.get("a", build("a")) is not a            # rebuilt on demand, and now b is the oldest
    assert build.calls == ["a", "b", "c", "a"] and list(cache.entries) == ["c", "a"]


def test_a_hit_makes_the_entry_the_most_recently_used(monkeypatch):
    monkeypatch.setenv("GLSDET_MAX_PLANS", "2")
    cache, build = PlanCache(), Builder()
    a, b = _fill(cache, build, "ab")
    assert cache.get("a", build("a")) is a
    cache.get("c", build("c"))
    assert list(cache.entries) == ["a", "c"] and cache.entries["a"] is a
    assert build.calls == ["a", "b", "c"]


def test_caps_below_one_keep_exactly_one_entry(monkeypatch):
    for cap in ("0", "-3"):
        monkeypatch.setenv("GLSDET_MAX_PLANS", cap)
        cache, build = PlanCache(), Builder()
        got = _fill(cache, build, "abc")
        assert list(cache.entries) == ["c"] and cache.entries["c"] is got[2], cap


def test_the_default_cap_is_24(monkeypatch):
    monkeypatch.delenv("GLSDET_MAX_PLANS", raising=False)
    cache, build = PlanCache(), Builder()
    _fill(cache, build, range(26))
    assert list(cache.entries) == list(range(2, 26))


def test_the_cap_is_read_at_insert_time(monkeypatch):
    monkeypatch.setenv("GLSDET_MAX_PLANS", "1")
    cache, build = PlanCache(), Builder()
    _fill(cache, build, "ab")
    assert list(cache.entries) == ["b"]
    monkeypatch.setenv("GLSDET_MAX_PLANS", "3")
    _fill(cache, build, "cd")
    assert list(cache.entries) == ["b", "c", "d"]
    monkeypatch.setenv("GLSDET_MAX_PLANS", "2")            # ... and lowering it evicts down to the new cap at the next insert
    _fill(cache, build, "e")
    assert list(cache.entries) == ["d", "e"]


def test_two_threads_missing_on_one_key_both_build_and_one_entry_stays():
    """The build runs outside the lock: both builders meet on a barrier INSIDE build (under the lock the second thread
    could not get there), both callers return their own plan, the later insert is the one the cache keeps."""
    cache, barrier, got = PlanCache(), threading.Barrier(2), {}

    def build():
        barrier.wait(timeout=5)
        return object()

    def worker(i):
        got[i] = cache.get("k", build)

    threads = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=5)
    assert not any(t.is_alive() for t in threads), "deadlock: a builder waited for the cache lock"
    assert set(got) == {0, 1} and got[0] is not got[1]
    assert list(cache.entries) == ["k"] and cache.entries["k"] in (got[0], got[1])
    assert cache.get("k", build) is cache.entries["k"]       # a hit: build (and its barrier) is not called again


def test_the_module_imports_without_torch_and_without_the_hip_library():
    code = ("import sys; import glsdet_amd.plans; "
            "bad = [m for m in ('torch', 'glsdet_amd._lib', 'glsdet_amd.engine') if m in sys.modules]; "
            "assert not bad, bad")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, timeout=60)
