"""--plane-clusters in the driver's plan (hc-mvs_amd/host/driver_plan.h) on the CPU: off by default, with --plane-priors 1 it feeds
--ransac-cluster into cluster_mul (10 when absent, as in the reference) and the "read and unused" note goes; without it the note stays; the
three errors; the option lives in a third table of its own and the two others are what they were.  tests/driver_plane_cluster_shim.cpp is
compiled with g++ alone: no HIP, no library."""
import ctypes as C
import os
import subprocess

import pytest

import test_driver_plan as DP

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "driver_plane_cluster_shim.cpp")
HOST = os.path.join(ROOT, "hc-mvs_amd", "host")
HDRS = [os.path.join(HOST, "driver_plan.h"), os.path.join(HOST, "scene_io.h"), os.path.join(ROOT, "include", "hcmvs_hip.h")]
LIB_PATH = os.path.join(HERE, "libdriver_plane_cluster_shim.so")
OK, USAGE, ERROR = 0, 1, 2
UNUSED = "--ransac-cluster is read and unused"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in [SRC] + HDRS):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    L.dpc_parse.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    L.dpc_parse.restype = C.c_char_p
    L.dpc_tables.argtypes = [C.c_int]
    L.dpc_tables.restype = C.c_char_p
    L.dpc_usage.restype = C.c_char_p
    return L


def parse(lib, *args):
    argv = [b"DensifyPointCloud", b"-i", b"x.mvs"] + [a.encode() for a in args]
    o = dict(notes=[])
    for line in lib.dpc_parse(len(argv), (C.c_char_p * len(argv))(*argv)).decode().splitlines():
        k, v = line.split("=", 1)
        if k == "note":
            o["notes"].append(v)
        else:
            o[k] = v
    return o


def test_defaults(lib):
    o = parse(lib)
    assert int(o["result"]) == OK and int(o["planeClusters"]) == 0 and float(o["ransacCluster"]) == 10.0 and float(o["cluster_mul"]) == 0.0 and o["notes"] == []
    o = parse(lib, "--plane-priors", "1")
    assert int(o["result"]) == OK and int(o["planeClusters"]) == 0 and float(o["cluster_mul"]) == 0.0 and o["notes"] == []
    assert float(parse(lib, "--plane-priors", "1", "--plane-clusters", "0", "--ransac-cluster", "3")["cluster_mul"]) == 0.0


def test_the_switch_feeds_ransac_cluster_into_cluster_mul(lib):
    o = parse(lib, "--plane-priors", "1", "--plane-clusters", "1", "--ransac-cluster", "3")
    assert int(o["result"]) == OK and int(o["planeClusters"]) == 1 and float(o["cluster_mul"]) == 3.0 and float(o["epsilon_mul"]) == 2.0
    o = parse(lib, "--plane-priors", "1", "--plane-clusters=1")
    assert int(o["result"]) == OK and float(o["cluster_mul"]) == 10.0                                # the reference's default
    assert float(parse(lib, "--plane-priors", "1", "--plane-clusters", "1", "--ransac-cluster", "7")["cluster_mul"]) == 7.0   # what the authors run


def test_the_note_is_absent_with_the_switch_and_present_without_it(lib):
    assert parse(lib, "--plane-priors", "1", "--plane-clusters", "1", "--ransac-cluster", "3")["notes"] == []
    for extra in ([], ["--plane-clusters", "0"]):
        notes = parse(lib, "--plane-priors", "1", "--ransac-cluster", "3", *extra)["notes"]
        assert len(notes) == 1 and notes[0].startswith(UNUSED)
    assert parse(lib, "--plane-priors", "1", "--ransac-cluster", "3", "-v", "1")["notes"] == []
    assert parse(lib, "--ransac-cluster", "3")["notes"] == []                                        # without the generation there is nothing to note


def test_the_three_errors(lib):
    o = parse(lib, "--plane-clusters", "1")
    assert int(o["result"]) == ERROR and "--plane-clusters" in o["err"] and "--plane-priors" in o["err"]
    o = parse(lib, "--plane-priors", "0", "--plane-clusters", "1", "--ransac-cluster", "3")
    assert int(o["result"]) == ERROR and "--plane-clusters" in o["err"] and "--plane-priors" in o["err"]
    for v in ("0", "-2", "nan", "inf", "x"):
        o = parse(lib, "--plane-priors", "1", "--plane-clusters", "1", "--ransac-cluster", v)
        assert int(o["result"]) == ERROR and "--ransac-cluster" in o["err"], v
        assert int(parse(lib, "--plane-priors", "1", "--ransac-cluster", v)["result"]) == OK         # read and unused without the switch, as before
    for v in ("2", "-1", "7"):
        o = parse(lib, "--plane-priors", "1", "--plane-clusters", v)
        assert int(o["result"]) == ERROR and "--plane-clusters" in o["err"], v
    assert int(parse(lib, "--plane-cluster", "1")["result"]) == ERROR                                 # unknown options stay errors


def test_the_option_tables_and_the_usage(lib):
    assert lib.dpc_tables(2).decode().split() == ["--plane-clusters"]
    assert lib.dpc_tables(0).decode().split() == list(DP.KNOWN)
    assert lib.dpc_tables(1).decode().split() == ["--depth-priors", "--plane-priors", "--export-priors"]
    usage = lib.dpc_usage().decode()
    assert "--plane-clusters 0|1" in usage and "--ransac-cluster" in usage
