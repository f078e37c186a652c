"""CPU: the free lists of the streaming interface's device blocks (rvtests_amd/csrc/block_pool.h through the host test
harness): which free block a gene gets, with what capacity it comes back, and what the trim keeps.  The move-only lease on
top of it is exercised by a stand-alone program under the address and undefined-behaviour sanitizers
(tools/block_lease_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import hc

KB = 1024


class Pool:
    def __init__(self):
        L = hc.lib()
        L.hc_pool_new.restype = C.c_void_p
        L.hc_pool_delete.argtypes = [C.c_void_p]
        L.hc_pool_give.argtypes = [C.c_void_p, C.c_size_t, C.c_longlong]
        L.hc_pool_take.restype = C.c_longlong
        L.hc_pool_take.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_size_t)]
        L.hc_pool_entries.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_longlong), C.c_int]
        L.hc_pool_trim.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_longlong), C.c_int]
        L.hc_pool_lease.restype = C.c_longlong
        L.hc_pool_lease.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_longlong, C.c_int, C.POINTER(C.c_size_t),
                                    C.POINTER(C.c_int)]
        self.L, self.p = L, L.hc_pool_new()

    def close(self):
        self.L.hc_pool_delete(self.p)

    def give(self, nbytes, name):
        self.L.hc_pool_give(self.p, nbytes, name)

    def take(self, need, bounded):
        b = C.c_size_t(0)
        name = self.L.hc_pool_take(self.p, need, int(bounded), C.byref(b))
        return name, b.value

    def entries(self):
        b, ids = (C.c_size_t * 64)(), (C.c_longlong * 64)()
        n = self.L.hc_pool_entries(self.p, b, ids, 64)
        return [(ids[i], b[i]) for i in range(n)]

    def trim(self, max_bytes, max_count):
        freed = (C.c_longlong * 64)()
        n = self.L.hc_pool_trim(self.p, max_bytes, max_count, freed, 64)
        return [freed[i] for i in range(n)]

    def lease(self, need, bounded, fresh_name, keep):
        b, fresh = C.c_size_t(0), C.c_int(0)
        name = self.L.hc_pool_lease(self.p, need, int(bounded), fresh_name, int(keep), C.byref(b), C.byref(fresh))
        return name, b.value, bool(fresh.value)


@pytest.fixture
def pool():
    p = Pool()
    yield p
    p.close()


def test_the_smallest_fitting_block_is_chosen(pool):
    for name, kb in ((1, 64), (2, 16), (3, 40), (4, 24), (5, 24)):
        pool.give(kb * KB, name)
    assert pool.take(20 * KB, False) == (4, 24 * KB)           # 24 KB is the smallest that holds 20; the first of two equals
    assert pool.take(20 * KB, False) == (5, 24 * KB)
    assert pool.take(16 * KB, False) == (2, 16 * KB)           # an exact fit
    assert pool.take(20 * KB, False) == (3, 40 * KB)
    assert pool.take(65 * KB, False) == (0, 0)                 # nothing fits: the caller allocates
    assert pool.entries() == [(1, 64 * KB)]


def test_the_four_times_bound_of_packed_blocks(pool):
    pool.give(40 * KB + 1, 1)
    assert pool.take(10 * KB, True) == (0, 0)                  # one byte more than 4 x the need: skipped
    assert pool.entries() == [(1, 40 * KB + 1)]
    pool.give(40 * KB, 2)
    assert pool.take(10 * KB, True) == (2, 40 * KB)            # exactly 4 x: taken
    assert pool.take(10 * KB, False) == (1, 40 * KB + 1)       # without the bound the large one serves


def test_a_returned_block_keeps_its_capacity(pool):
    pool.give(40 * KB, 7)
    # a lease that asks for 17 KB gets the 40 KB block, and dropped (an early return) it goes back as 40 KB
    assert pool.lease(17 * KB, True, 99, keep=False) == (7, 40 * KB, False)
    assert pool.entries() == [(7, 40 * KB)]
    # released to the caller (a queued gene) nothing goes back
    assert pool.lease(17 * KB, True, 99, keep=True) == (7, 40 * KB, False)
    assert pool.entries() == []
    # nothing pooled: the block is allocated, of the size asked for, fresh (the caller clears it), and pooled when dropped
    assert pool.lease(3 * KB, True, 99, keep=False) == (99, 3 * KB, True)
    assert pool.entries() == [(99, 3 * KB)]


def test_the_trim_frees_from_the_back_until_both_bounds_hold(pool):
    for name, kb in ((1, 10), (2, 20), (3, 30), (4, 40), (5, 50)):
        pool.give(kb * KB, name)
    assert pool.trim(150 * KB, 5) == []                        # both bounds hold
    assert pool.trim(70 * KB, 5) == [5, 4]                     # 150 -> 100 -> 60 KB
    assert pool.entries() == [(1, 10 * KB), (2, 20 * KB), (3, 30 * KB)]
    assert pool.trim(70 * KB, 2) == [3]                        # the count bound alone
    assert pool.trim(2 ** 64 - 1, 1) == [2]                    # no byte bound (the packed pool)
    assert pool.trim(5 * KB, 4) == [1]                         # the byte bound alone empties it
    assert pool.entries() == []


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer runs belong on machines without a GPU")
def test_the_lease_returns_its_block_once_on_every_way_out(tmp_path):
    """tools/block_lease_check.cpp with fake allocate / free callbacks, under -fsanitize=address,undefined: every early exit
    returns the block exactly once, a released lease returns nothing, no block is freed twice or lost."""
    gxx = shutil.which("g++")
    assert gxx
    exe = str(tmp_path / "block_lease_check")
    subprocess.check_call([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", hc.CSRC, os.path.join(hc.ROOT, "tools", "block_lease_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "block lease: ok" in r.stdout, r.stdout + r.stderr
