"""--speckle-size and --speckle-diff of the driver's plan (hc-mvs_amd/host/driver_plan.h) on the CPU: both parse into the options, the
defaults are 0 (off) and 0.01f * 0.7f, a negative size and a difference that is not a finite number > 0 are parse errors, they stand in
a table of their own (the existing tables are what they were) and in the usage text, which names upstream's 100.
tests/driver_speckle_shim.cpp is compiled with g++ alone: no HIP, no library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_driver_plan as DP

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "driver_speckle_shim.cpp")
HOST = os.path.join(ROOT, "hc-mvs_amd", "host")
HDRS = [os.path.join(HOST, "driver_plan.h"), os.path.join(HOST, "scene_io.h"), os.path.join(ROOT, "include", "hcmvs_hip.h")]
LIB_PATH = os.path.join(HERE, "libdriver_speckle_shim.so")
OK, USAGE, ERROR = 0, 1, 2
DEFAULT_BITS = int((np.float32(0.01) * np.float32(0.7)).view(np.uint32))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in [SRC] + HDRS):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    L.dps_parse.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    L.dps_parse.restype = C.c_char_p
    L.dps_tables.argtypes = [C.c_int]
    L.dps_tables.restype = C.c_char_p
    L.dps_usage.restype = C.c_char_p
    return L


def parse(lib, *args):
    argv = [b"DensifyPointCloud"] + [a.encode() for a in args]
    return dict(line.split("=", 1) for line in lib.dps_parse(len(argv), (C.c_char_p * len(argv))(*argv)).decode().splitlines())


def bits(x):
    return int(np.float32(x).view(np.uint32))


def test_the_default_is_off(lib):
    for extra in ([], ["--n-nOptimize", "3"], ["--n-filter", "1"], ["--fusion-mode", "1"]):
        o = parse(lib, "-i", "x.mvs", *extra)
        assert int(o["result"]) == OK and int(o["speckleSize"]) == 0 and int(o["speckleDiffBits"]) == DEFAULT_BITS
    # the REMOVE_SPECKLES bit of --n-nOptimize gates the fork's own chain, as before, and nothing of this filter
    assert int(parse(lib, "-i", "x.mvs", "--n-nOptimize", "1")["postFilter"]) == 1 and int(parse(lib, "-i", "x.mvs", "--n-nOptimize", "1")["speckleSize"]) == 0


@pytest.mark.parametrize("n", [0, 1, 100, 5000])
def test_the_size_parses(lib, n):
    o = parse(lib, "-i", "x.mvs", "--speckle-size", str(n))
    assert int(o["result"]) == OK and int(o["speckleSize"]) == n and int(o["speckleDiffBits"]) == DEFAULT_BITS and int(o["notes"]) == 0
    o = parse(lib, "-i", "x.mvs", "--speckle-size=%d" % n, "--n-filter", "2", "--n-nOptimize", "3")
    assert int(o["result"]) == OK and int(o["speckleSize"]) == n and int(o["nFilter"]) == 2 and int(o["postFilter"]) == 1


@pytest.mark.parametrize("f", ["0.007", "0.01", "1e-4", "0.5", "3"])
def test_the_difference_parses(lib, f):
    o = parse(lib, "-i", "x.mvs", "--speckle-size", "100", "--speckle-diff", f)
    assert int(o["result"]) == OK and int(o["speckleDiffBits"]) == bits(float(f))
    o = parse(lib, "-i", "x.mvs", "--speckle-diff=" + f)                    # read without a size, and then unused
    assert int(o["result"]) == OK and int(o["speckleSize"]) == 0 and int(o["speckleDiffBits"]) == bits(float(f))


def test_parse_errors(lib):
    for bad in ("-1", "-100"):
        o = parse(lib, "-i", "x.mvs", "--speckle-size", bad)
        assert int(o["result"]) == ERROR and "--speckle-size" in o["err"], bad
    for bad in ("0", "-0.007", "nan", "inf", "-inf"):
        for size in ("0", "100"):
            o = parse(lib, "-i", "x.mvs", "--speckle-size", size, "--speckle-diff", bad)
            assert int(o["result"]) == ERROR and "--speckle-diff" in o["err"], bad
    assert int(parse(lib, "-i", "x.mvs", "--speckle-size")["result"]) == ERROR                    # the value is required
    assert int(parse(lib, "-i", "x.mvs", "--speckle-sizes", "1")["result"]) == ERROR              # unknown options stay errors
    # runs that are no densify run read both and do nothing with them, as they do with the other options
    assert int(parse(lib, "-i", "mesh.ply", "--sample-mesh", "5", "--speckle-size", "-4")["result"]) == OK


def test_a_table_of_its_own_and_the_usage_text(lib):
    assert lib.dps_tables(0).decode().split() == ["--speckle-size", "--speckle-diff"]
    assert lib.dps_tables(1).decode().split() == list(DP.KNOWN)                                   # dp_known_options: unchanged
    assert lib.dps_tables(2).decode().split() == ["--plane-refit"]
    usage = lib.dps_usage().decode()
    assert "--speckle-size n" in usage and "100" in usage[usage.index("--speckle-size n"):usage.index("--n-filter 0|1|2")]
    assert "--speckle-diff" in usage and usage.index("--plane-refit n") < usage.index("--speckle-size n") < usage.index("--n-filter 0|1|2")
