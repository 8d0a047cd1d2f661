"""helper: the sweep launch plan (hc-mvs_amd/csrc/sweep_plan.h) through tests/sweep_plan_shim.cpp, compiled with g++ alone -- no HIP, no
library.  Shared by test_sweep_plan.py, test_sweep_matrix_plan.py and test_gpu_sweep_matrix.py."""
import ctypes as C
import itertools
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sweep_plan_shim.cpp")
HDR = os.path.join(os.path.dirname(HERE), "hc-mvs_amd", "csrc", "sweep_plan.h")
LIB_PATH = os.path.join(HERE, "libsweep_plan_shim.so")

AUTO, PER_SWEEP, ONE = 0, 1, 2
FLAGS = ("big", "two", "pack", "hint", "mask", "spread")

_lib = None


def load():
    """the shim, compiled when it is missing or older than its sources"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in (SRC, HDR)):
            subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
        _lib = C.CDLL(LIB_PATH)
    return _lib


def _variant(a):
    d = {"nw": a[0], "exists": bool(a[7])}
    d.update({f: bool(a[1 + i]) for i, f in enumerate(FLAGS)})
    return d


def resolve(lib, requested, V, big=False, hint=False, mask=False, spread=False):
    out = (C.c_int * 8)()
    lib.sp_resolve(requested, V, int(big), int(hint), int(mask), int(spread), out)
    return _variant(out)


def image(w, h, n_src=8, border=7, hint=False, mask=False, spread=False):
    return (h - 2 * border, w - 2 * border, n_src, int(hint), int(mask), int(spread))


def plan(lib, items, n_sweeps=8, big=False, n_cu=256, launches=AUTO, segment=-1, waves=0):
    flat = (C.c_int * (6 * len(items)))(*itertools.chain.from_iterable(items))
    cap = max(n_sweeps, 1)
    out = (C.c_int * (13 * cap))()
    n = lib.sp_plan(flat, len(items), int(big), n_sweeps, n_cu, (C.c_int * 3)(launches, segment, waves), out, cap)
    assert 0 <= n <= cap
    res = []
    for i in range(n):
        a = out[13 * i:13 * i + 13]
        d = dict(first=a[0], count=a[1], segLen=a[2], tickets=a[3], grid=a[4])
        d.update(_variant(a[5:]))
        res.append(d)
    return res
