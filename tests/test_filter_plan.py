"""How hcmvs_filter_sequence cuts its images into batches and what it does when the z-buffer keys of a batch cannot be allocated
(hc-mvs_amd/csrc/filter_plan.h) on the CPU.  tests/filter_plan_shim.cpp is compiled with g++ alone: no HIP, no library."""
import ctypes as C
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "filter_plan_shim.cpp")
HDR = os.path.join(os.path.dirname(HERE), "hc-mvs_amd", "csrc", "filter_plan.h")
LIB_PATH = os.path.join(HERE, "libfilter_plan_shim.so")
U64 = C.c_ulonglong
NO_BUDGET = 2 ** 64 - 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in (SRC, HDR)):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    L.fp_parse.argtypes = [C.c_char_p, U64, C.POINTER(U64)]
    L.fp_plan.argtypes = [C.POINTER(U64), C.c_int, U64, U64, C.POINTER(U64), C.POINTER(U64)]
    L.fp_retry.argtypes = [C.POINTER(U64), C.c_int, U64, U64, U64, C.c_int, C.POINTER(U64)]
    return L


def plan(lib, need, budget=NO_BUDGET, cap=0):
    first = (U64 * (len(need) + 1))(); kb = U64()
    n = lib.fp_plan((U64 * max(len(need), 1))(*need), len(need), budget, cap, first, C.byref(kb))
    return list(first[:n]), kb.value


def retry(lib, need, avail, budget=NO_BUDGET, cap=0, max_tries=200):
    kb = U64()
    t = lib.fp_retry((U64 * len(need))(*need), len(need), budget, cap, avail, max_tries, C.byref(kb))
    return t, kb.value


def test_the_knob_is_a_positive_number_or_all(lib):
    cap = U64()
    assert lib.fp_parse(None, 5, C.byref(cap)) == 1 and cap.value == 0
    assert lib.fp_parse(b"all", 5, C.byref(cap)) == 1 and cap.value == 5
    assert lib.fp_parse(b"7", 5, C.byref(cap)) == 1 and cap.value == 7
    for bad in (b"7abc", b"", b"0", b"-3", b"ALL", b"1.5", b" "):
        assert lib.fp_parse(bad, 5, C.byref(cap)) == 0, bad


def test_batches_by_budget_and_by_cap(lib):
    need = [10, 10, 10, 10, 10]
    assert plan(lib, need) == ([0, 5], 50)
    assert plan(lib, need, budget=25) == ([0, 2, 4, 5], 20)
    assert plan(lib, need, cap=1) == ([0, 1, 2, 3, 4, 5], 10)
    assert plan(lib, need, cap=2, budget=30) == ([0, 2, 4, 5], 20)
    assert plan(lib, need, budget=3) == ([0, 1, 2, 3, 4, 5], 10)      # an image beyond the budget: a batch of its own
    assert plan(lib, [80, 20, 20], budget=40) == ([0, 1, 3], 80)
    assert plan(lib, [2 ** 63, 2 ** 63, 5], budget=NO_BUDGET - 1) == ([0, 1, 3], 2 ** 63 + 5)   # no overflow in the sum


def test_retry_ends_when_the_largest_image_does_not_fit(lib):
    """one image with 8 neighbours followed by two with 2 each: once the batches are [80] and [20, 20], halving the budget no longer
    changes the plan -- the call must give up, not try the same allocation for ever"""
    tries, kb = retry(lib, [80, 20, 20], avail=70)
    assert kb == 0 and tries <= 3
    tries, kb = retry(lib, [80, 20, 20], avail=70, budget=40)
    assert kb == 0 and tries == 1
    tries, kb = retry(lib, [80, 20, 20], avail=80)
    assert kb == 80 and tries == 2                                    # 120 fails, 80 | 40 fits
    tries, kb = retry(lib, [10] * 64, avail=35)
    assert kb == 20 and tries == 6                                    # 640, 320, 160, 80, 40 fail; 20 fits
    tries, kb = retry(lib, [10] * 64, avail=9)
    assert kb == 0 and tries <= 8
    tries, kb = retry(lib, [10] * 8, avail=25, cap=4)                 # a forced batch that does not fit shrinks, and the cap still holds
    assert kb == 20 and tries == 2


def test_retry_always_ends_and_finds_a_plan_when_every_image_fits(lib):
    rnd = random.Random(4)
    for _ in range(300):
        need = [rnd.choice([1, 2, 8]) * rnd.choice([100, 400, 1000]) for _ in range(rnd.randint(1, 40))]
        avail = rnd.randint(50, 12000)
        cap = rnd.choice([0, 0, 1, 3, 100])
        tries, kb = retry(lib, need, avail, budget=rnd.choice([NO_BUDGET, 5000, 900]), cap=cap)
        assert tries <= 70, (need, avail)                             # keyBytes falls by half or to the largest image: log2 steps
        if max(need) <= avail:
            assert 0 < kb <= avail, (need, avail)
        else:
            assert kb == 0
