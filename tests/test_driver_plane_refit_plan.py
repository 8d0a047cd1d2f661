"""--plane-refit of the driver's plan (hc-mvs_amd/host/driver_plan.h) on the CPU: the option parses into the options and reaches refit_iters of
the detection's parameters, its range is 0 .. 16, it needs --plane-priors 1, its default is 0, it stands in a table of its own (the
existing tables are what they were) and in the usage text.  tests/driver_plane_refit_shim.cpp is compiled with g++ alone: no HIP, no
library."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "driver_plane_refit_shim.cpp")
HOST = os.path.join(ROOT, "hc-mvs_amd", "host")
HDRS = [os.path.join(HOST, "driver_plan.h"), os.path.join(HOST, "scene_io.h"), os.path.join(ROOT, "include", "hcmvs_hip.h")]
LIB_PATH = os.path.join(HERE, "libdriver_plane_refit_shim.so")
OK, USAGE, ERROR = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in [SRC] + HDRS):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    L.dpr_parse.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    L.dpr_parse.restype = C.c_char_p
    L.dpr_tables.argtypes = [C.c_int]
    L.dpr_tables.restype = C.c_char_p
    L.dpr_usage.restype = C.c_char_p
    return L


def parse(lib, *args):
    argv = [b"DensifyPointCloud"] + [a.encode() for a in args]
    return dict(line.split("=", 1) for line in lib.dpr_parse(len(argv), (C.c_char_p * len(argv))(*argv)).decode().splitlines())


def test_the_default_is_no_refit(lib):
    for extra in ([], ["--plane-priors", "1"], ["--plane-priors", "1", "--plane-clusters", "1"]):
        o = parse(lib, "-i", "x.mvs", *extra)
        assert int(o["result"]) == OK and int(o["planeRefit"]) == 0 and int(o["refit_iters"]) == 0


@pytest.mark.parametrize("n", [0, 1, 4, 16])
def test_the_option_reaches_the_parameters(lib, n):
    o = parse(lib, "-i", "x.mvs", "--plane-priors", "1", "--plane-refit", str(n))
    assert int(o["result"]) == OK and int(o["planeRefit"]) == n == int(o["refit_iters"]) and float(o["cluster_mul"]) == 0 and int(o["notes"]) == 0
    o = parse(lib, "-i", "x.mvs", "--plane-priors", "1", "--plane-refit=%d" % n, "--plane-clusters", "1", "--ransac-cluster", "7")
    assert int(o["result"]) == OK and int(o["refit_iters"]) == n and float(o["cluster_mul"]) == 7.0


def test_the_range_is_0_to_16(lib):
    for bad in ("-1", "17", "100"):
        o = parse(lib, "-i", "x.mvs", "--plane-priors", "1", "--plane-refit", bad)
        assert int(o["result"]) == ERROR and "--plane-refit" in o["err"] and "16" in o["err"], bad
        o = parse(lib, "-i", "x.mvs", "--plane-refit", bad)
        assert int(o["result"]) == ERROR and "--plane-refit" in o["err"]


def test_it_needs_the_generated_priors(lib):
    for extra in ([], ["--plane-priors", "0"], ["--depth-priors", "P"]):
        o = parse(lib, "-i", "x.mvs", "--plane-refit", "4", *extra)
        assert int(o["result"]) == ERROR and "--plane-refit" in o["err"] and "--plane-priors" in o["err"]
    assert int(parse(lib, "-i", "x.mvs", "--plane-refit", "0")["result"]) == OK                  # 0 asks for nothing
    assert int(parse(lib, "-i", "x.mvs", "--plane-refit")["result"]) == ERROR                    # the value is required
    assert int(parse(lib, "-i", "x.mvs", "--plane-refits", "1")["result"]) == ERROR              # unknown options stay errors
    # runs that are no densify run read it and do nothing with it, as they do with the other options
    assert int(parse(lib, "-i", "mesh.ply", "--sample-mesh", "5", "--plane-refit", "40")["result"]) == OK


def test_a_table_of_its_own_and_the_usage_text(lib):
    assert lib.dpr_tables(0).decode().split() == ["--plane-refit"]
    assert lib.dpr_tables(1).decode().split() == ["--plane-clusters"]
    assert lib.dpr_tables(2).decode().split() == ["--depth-priors", "--plane-priors", "--export-priors"]
    usage = lib.dpr_usage().decode()
    assert "--plane-refit n" in usage and "0 .. 16" in usage and usage.index("--plane-clusters 0|1") < usage.index("--plane-refit n") < usage.index("--n-filter 0|1|2")
