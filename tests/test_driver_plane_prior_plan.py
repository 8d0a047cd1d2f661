"""The plane-prior options of the driver's plan (hc-mvs_amd/host/driver_plan.h) on the CPU: --plane-priors, --export-priors and the --ransac-*
options parse into the options and the detection's parameters, the exclusive combinations are errors that name both options, the schedule is
that of --depth-priors, and kKnownOptions and the --use-semantic note are what they were.  tests/driver_plane_prior_shim.cpp is compiled with
g++ alone: no HIP, no library."""
import ctypes as C
import os
import subprocess

import pytest

import test_driver_plan as DP

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "driver_plane_prior_shim.cpp")
HOST = os.path.join(ROOT, "hc-mvs_amd", "host")
HDRS = [os.path.join(HOST, "driver_plan.h"), os.path.join(HOST, "scene_io.h"), os.path.join(ROOT, "include", "hcmvs_hip.h")]
LIB_PATH = os.path.join(HERE, "libdriver_plane_prior_shim.so")
OK, USAGE, ERROR = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in [SRC] + HDRS):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    L.dpp_parse.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    L.dpp_parse.restype = C.c_char_p
    L.dpp_schedule.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.dpp_schedule.restype = None
    L.dpp_path.argtypes = [C.c_char_p, C.c_uint]
    L.dpp_path.restype = C.c_char_p
    L.dpp_tables.argtypes = [C.c_int]
    L.dpp_tables.restype = C.c_char_p
    return L


def parse(lib, *args):
    argv = [b"DensifyPointCloud"] + [a.encode() for a in args]
    o = dict(notes=[])
    for line in lib.dpp_parse(len(argv), (C.c_char_p * len(argv))(*argv)).decode().splitlines():
        k, v = line.split("=", 1)
        if k == "note":
            o["notes"].append(v)
        else:
            o[k] = v
    return o


def test_defaults(lib):
    o = parse(lib, "-i", "x.mvs")
    assert int(o["result"]) == OK and int(o["planePriors"]) == 0 and o["exportPriors"] == "" and o["notes"] == []
    assert (float(o["probability"]), float(o["epsilon_mul"]), float(o["min_points_div"]), int(o["seed"]), int(o["region_label"])) == (pytest.approx(0.01), 2.0, 80.0, 1234, 255)


def test_the_options_parse_and_feed_the_parameters(lib):
    o = parse(lib, "-i", "x.mvs", "--plane-priors", "1", "--export-priors=/data/P", "--ransac-probability", "0.05", "--ransac-epsilon", "1.5", "--ransac-min-points", "40",
              "--seed", "99", "--ransac-cluster", "3")
    assert int(o["result"]) == OK and int(o["planePriors"]) == 1 and o["exportPriors"] == "/data/P"
    assert (float(o["probability"]), float(o["epsilon_mul"]), float(o["min_points_div"]), int(o["seed"])) == (pytest.approx(0.05), 1.5, 40.0, 99)
    assert (int(o["n_neighbors"]), int(o["max_rounds"]), int(o["region_label"])) == (10, 256, 255)      # untouched, and the label of the reference's region
    assert len(o["notes"]) == 1 and "--ransac-cluster" in o["notes"][0] and "unused" in o["notes"][0]
    assert parse(lib, "-i", "x.mvs", "--plane-priors", "1", "--ransac-cluster", "3", "-v", "1")["notes"] == []
    assert parse(lib, "-i", "x.mvs", "--ransac-cluster", "3")["notes"] == []                             # without the generation there is nothing to note
    assert int(parse(lib, "-i", "x.mvs", "--plane-priors", "0", "--n-viewspread", "1")["result"]) == OK
    assert lib.dpp_path(b"/data/P", 12).decode() == "/data/P/depth0012.prior.dmap"


def test_the_refused_combinations_name_both_options(lib):
    for extra, word in ((["--depth-priors", "p"], "--depth-priors"), (["--n-viewspread", "1"], "--n-viewspread"), (["--restore-hypothesis", "1"], "--restore-hypothesis")):
        o = parse(lib, "-i", "x.mvs", "--plane-priors", "1", *extra)
        assert int(o["result"]) == ERROR and word in o["err"] and "--plane-priors" in o["err"]
    o = parse(lib, "-i", "x.mvs", "--export-priors", "P")
    assert int(o["result"]) == ERROR and "--export-priors" in o["err"] and "--plane-priors" in o["err"]
    for extra, word in ((["--plane-priors", "2"], "--plane-priors"), (["--ransac-probability", "0"], "--ransac-probability"), (["--ransac-probability", "1"], "--ransac-probability"),
                        (["--ransac-epsilon", "0"], "--ransac-epsilon"), (["--ransac-min-points", "-3"], "--ransac-min-points"), (["--n-para_prior", "1.5"], "--n-para_prior"),
                        (["--sigma-prior", "0"], "--sigma-prior"), (["--n-photo2geo", "-1"], "--n-photo2geo")):
        o = parse(lib, "-i", "x.mvs", "--plane-priors", "1", *extra)
        assert int(o["result"]) == ERROR and word in o["err"], extra
    assert int(parse(lib, "-i", "x.mvs", "--ransac-probability", "0")["result"]) == OK                  # read and unused without the generation, as before
    assert int(parse(lib, "-i", "x.mvs", "--plane-prior", "1")["result"]) == ERROR                      # unknown options stay errors


def test_the_schedule_is_that_of_the_depth_priors(lib):
    out = (C.c_int * 2)()
    for n_ext in (1, 2, 3, 4):
        for it in range(n_ext):
            lib.dpp_schedule(1, n_ext, it, out)
            assert (out[0], out[1]) == (int(it == n_ext - 2), int(n_ext < 2))
            lib.dpp_schedule(0, n_ext, it, out)
            assert (out[0], out[1]) == (0, 0)


def test_the_option_tables(lib):
    known = lib.dpp_tables(0).decode().split()
    assert "--plane-priors" not in known and "--export-priors" not in known and "--depth-priors" not in known
    assert known == list(DP.KNOWN)
    assert lib.dpp_tables(1).decode().split() == ["--depth-priors", "--plane-priors", "--export-priors"]


def test_use_semantic_keeps_its_note(lib):
    for extra in ([], ["--plane-priors", "1"]):
        o = parse(lib, "-i", "x.mvs", "--use-semantic", "1", *extra)
        assert int(o["result"]) == OK
        assert o["notes"] == ["--use-semantic is not available in this build (defined subset); treated as 0 (prior depth maps made elsewhere can be supplied with "
                              "--depth-priors <folder>)"]
