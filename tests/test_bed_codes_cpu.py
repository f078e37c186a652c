"""What every reader of resident .bed rows shares (rvtests_amd/csrc/rvt_bed_codes.h through hc_bed_*) against a few lines of numpy:
the value of a code, the site pass on a row's four counts, the live masks, the population counts, the spread of a code byte into
byte lanes and the loaders of 4 and 16 bytes from any byte address; where V rows at an address lie in a matrix of known extent
(bed_span, the arithmetic under every range check of resident rows) against Python integers; and the loaders and bed_span once
more as a stand-alone program under the address and undefined-behaviour sanitizers (tools/bed_codes_check.cpp), the proof that
the loaders touch no byte outside [base, end) and that the row arithmetic overflows nowhere."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import fam_bed_cases
import hc

CALL_OF_CODE = np.array([0.0, -9.0, 1.0, 2.0])            # 00 -> 0, 01 -> missing, 10 -> 1, 11 -> 2


def lib():
    L = hc.lib()
    L.hc_bed_site.restype = C.c_double
    L.hc_bed_site.argtypes = [C.c_longlong] * 4 + [C.POINTER(C.c_longlong)]
    L.hc_bed_value.restype = C.c_double
    L.hc_bed_value.argtypes = [C.c_uint, C.c_double]
    for n in ("hc_bed_live_pairs", "hc_bed_live_lanes"):
        getattr(L, n).restype = C.c_uint
        getattr(L, n).argtypes = [C.c_longlong]
    L.hc_bed_counts16.restype = None
    L.hc_bed_counts16.argtypes = [C.c_uint, C.c_longlong, C.POINTER(C.c_int)]
    L.hc_bed_spread.restype = C.c_uint
    L.hc_bed_spread.argtypes = [C.c_uint, C.c_int]
    L.hc_bed_load4.restype = C.c_uint
    L.hc_bed_load4.argtypes = [C.c_void_p] + [C.c_longlong] * 3
    L.hc_bed_load16.restype = None
    L.hc_bed_load16.argtypes = [C.c_void_p] + [C.c_longlong] * 3 + [C.POINTER(C.c_uint)]
    return L


@pytest.fixture(scope="module")
def all_bytes():
    """One row whose byte b is b, packed by the project's own packer from the calls the format assigns to it: (bytes (256,),
    calls (256, 4), -9 = missing)."""
    b = np.arange(256)
    calls = CALL_OF_CODE[(b[:, None] >> (2 * np.arange(4))) & 3]
    row = fam_bed_cases.pack(np.asfortranarray(calls.reshape(-1, 1)))[0]
    assert np.array_equal(row, b.astype(np.uint8))         # sample i in bits 2 (i & 3) of byte i >> 2
    return row, calls


def test_value_of_every_code():
    L = lib()
    for q in range(4):
        for fill in (0.0, 0.3125, 1.0, 2.0 - 1.0 / 3.0):
            want = fill if CALL_OF_CODE[q] < 0 else CALL_OF_CODE[q]
            assert L.hc_bed_value(q, fill) == want


def test_live_masks():
    L = lib()
    for left in range(-3, 21):
        k = min(max(left, 0), 16)
        assert L.hc_bed_live_pairs(left) == sum(1 << (2 * e) for e in range(k))
        k = min(max(left, 0), 4)
        assert L.hc_bed_live_lanes(left) == sum(1 << (8 * e) for e in range(k))


def test_spread_and_counts_of_every_byte(all_bytes):
    """All 256 bytes x `left` 0 .. 17: the byte in every position of a dword whose other bytes are other bytes of the row."""
    L = lib()
    row, calls = all_bytes
    for b in range(256):
        idx = np.array([b, (b * 7 + 3) & 255, (b * 13 + 101) & 255, 255 - b])
        for k in range(4):
            pos = np.roll(idx, k)                          # byte b sits in position k
            code = int(sum(int(row[p]) << (8 * j) for j, p in enumerate(pos)))
            lo, hi = L.hc_bed_spread(code, k), L.hc_bed_spread(code >> 1, k)
            for e in range(4):
                q = (b >> (2 * e)) & 3
                assert (lo >> (8 * e)) & 0xFF == (q & 1) and (hi >> (8 * e)) & 0xFF == (q >> 1)
            c16 = calls[pos].reshape(-1)                   # the 16 samples of the dword
            for left in range(18):
                live = c16[:min(left, 16)]
                n = (C.c_int * 4)(5, 6, 7, 8)              # (added to)
                L.hc_bed_counts16(code, left, n)
                assert list(n) == [5 + int((live == 0).sum()), 6 + int((live == 1).sum()), 7 + int((live == 2).sum()),
                                   8 + int((live < 0).sum())], (b, k, left)


SITE_ROWS = {                                              # n0, n1, n2, missing
    "nothing called": (0, 0, 0, 9),
    "one called sample": (0, 1, 0, 514),
    "ac == called": (3, 4, 3, 2),
    "ac == called + 1": (3, 3, 4, 0),
    "only n0": (12, 0, 0, 1),
    "only n1": (0, 12, 0, 0),
    "only n2": (0, 0, 12, 3),
    "n0 and n2 without n1": (5, 0, 7, 1),
    "a common row": (301, 170, 41, 3),
}


@pytest.mark.parametrize("name", list(SITE_ROWS))
def test_site_pass_on_the_edge_rows(name):
    n0, n1, n2, nm = SITE_ROWS[name]
    out = (C.c_longlong * 5)()
    mean = lib().hc_bed_site(n0, n1, n2, nm, out)
    called, ac = n0 + n1 + n2, n1 + 2 * n2
    assert list(out) == [called, ac, int((n0 > 0) + (n1 > 0) + (n2 > 0) >= 2), int(ac > called), nm]
    assert mean == (np.float64(ac) / np.float64(called) if called else 0.0)   # one division of the two integers as doubles
    if name == "ac == called":
        assert mean == 1.0 and out[3] == 0
    if name == "ac == called + 1":
        assert out[3] == 1


def test_loaders_at_every_alignment_and_distance_from_both_ends():
    """p at every alignment 0 .. 3, every distance 0 .. 24 behind `base` and in front of `end`: the value is the byte-wise read
    with zeros from `end` on, whatever lies outside [base, end)."""
    L = lib()
    rng = np.random.default_rng(515)
    buf = np.empty(128, dtype=np.uint8)
    addr = buf.ctypes.data
    w4 = (C.c_uint * 4)()
    for align in range(4):
        for db in range(25):
            off = 32 + (align - (addr + 32)) % 4           # (addr + off) & 3 == align, and off - 24 >= 0
            assert (addr + off) % 4 == align
            for de in range(25):
                base, end = off - db, off + de
                buf[:] = 0xFF
                buf[base:end] = rng.integers(0, 256, end - base, dtype=np.uint8)
                ext = np.concatenate([buf[off:end], np.zeros(16, dtype=np.uint8)])[:16]
                want = [int.from_bytes(ext[4 * k:4 * k + 4].tobytes(), "little") for k in range(4)]
                assert L.hc_bed_load4(addr, off, base, end) == want[0], (align, db, de)
                L.hc_bed_load16(addr, off, base, end, w4)
                assert list(w4) == want, (align, db, de)


OUTSIDE, OFF_ROW, LEAVES = -1, -2, -3


def span(base, nv, pitch, at, V):
    """bed_span in Python integers"""
    off = at - base
    if off < 0 or off >= nv * pitch:
        return OUTSIDE
    if off % pitch:
        return OFF_ROW
    return LEAVES if off // pitch + V > nv else off // pitch


@pytest.mark.parametrize("pitch", [1, 129, 125000])
@pytest.mark.parametrize("nv", [1, 2, 4099])
def test_span_of_rows_in_a_matrix(pitch, nv):
    """Where V rows at an address lie in a matrix of nv rows: every first row, V from 1 to one past the end, addresses around
    both ends, off the row boundaries and in the slack, bases near 2^47, and V = 2^30, 2^62 (no overflow: "leave the matrix")."""
    L = lib()
    L.hc_bed_span.restype = C.c_longlong
    L.hc_bed_span.argtypes = [C.c_ulonglong, C.c_longlong, C.c_longlong, C.c_ulonglong, C.c_longlong]
    L.hc_bed_pitch.restype = C.c_longlong
    L.hc_bed_pitch.argtypes = [C.c_longlong]
    assert [L.hc_bed_pitch(n) for n in (1, 4, 5, 515, 516, 517, 500000)] == [1, 1, 2, 129, 129, 130, 125000]
    slack = L.hc_bed_slack()
    assert slack == 16

    def same(base, at, V):
        got, want = L.hc_bed_span(base, nv, pitch, at, V), span(base, nv, pitch, at, V)
        assert got == want, (base, at - base, V, got, want)
        return got

    for base in (1 << 12, (1 << 47) - 4096, (1 << 47) - 1, (1 << 47) + 3):
        end = base + nv * pitch
        for first in range(nv):                                    # every first row
            at = base + first * pitch
            left = nv - first
            assert same(base, at, left) == first and same(base, at, left + 1) == LEAVES
            assert same(base, at, 1 << 30) == (first if left >= 1 << 30 else LEAVES)
            assert same(base, at, 1 << 62) == LEAVES and same(base, at, (1 << 63) - 1) == LEAVES
            if pitch > 1:
                assert same(base, at + 1, 1) == OFF_ROW and same(base, at + pitch - 1, 1) == OFF_ROW
        for first in sorted({0, nv // 2, nv - 1}):                 # V from 1 to one past the end
            for V in (range(1, nv - first + 2) if nv < 100 or first else range(1, nv + 2)):
                assert same(base, base + first * pitch, V) == (first if first + V <= nv else LEAVES)
        for at in (base - 1, base - pitch, end, end + 1, end + slack - 1, end + slack, end + pitch):
            for V in (1, nv, 1 << 62):
                assert same(base, at, V) == OUTSIDE


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer runs belong on machines without a GPU")
def test_the_loaders_touch_no_byte_outside_the_buffer(tmp_path):
    """tools/bed_codes_check.cpp under -fsanitize=address,undefined: heap buffers of exactly end - base bytes, every length
    1 .. 40, every offset; and bed_span over a few hundred cases against 128-bit arithmetic."""
    gxx = shutil.which("g++")
    assert gxx
    exe = str(tmp_path / "bed_codes_check")
    subprocess.check_call([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", hc.CSRC, os.path.join(hc.ROOT, "tools", "bed_codes_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "bed codes: ok" in r.stdout, r.stdout + r.stderr
