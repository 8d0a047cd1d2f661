"""The depth-prior options of the driver's plan (hc-mvs_amd/host/driver_plan.h) on the CPU: --sigma-prior, --n-para_prior, --n-photo2geo and
--depth-priors parse into the options, the exclusive combinations are errors, --use-semantic keeps its note, and the schedule helpers follow
the reference's.  tests/driver_prior_shim.cpp is compiled with g++ alone: no HIP, no library."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "driver_prior_shim.cpp")
HOST = os.path.join(ROOT, "hc-mvs_amd", "host")
HDRS = [os.path.join(HOST, "driver_plan.h"), os.path.join(HOST, "scene_io.h"), os.path.join(ROOT, "include", "hcmvs_hip.h")]
LIB_PATH = os.path.join(HERE, "libdriver_prior_shim.so")
OK, USAGE, ERROR = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in [SRC] + HDRS):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    L.dq_parse.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    L.dq_parse.restype = C.c_char_p
    L.dq_schedule.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.dq_schedule.restype = None
    L.dq_path.argtypes = [C.c_char_p, C.c_uint]
    L.dq_path.restype = C.c_char_p
    return L


def parse(lib, *args):
    argv = [b"DensifyPointCloud"] + [a.encode() for a in args]
    o = dict(notes=[])
    for line in lib.dq_parse(len(argv), (C.c_char_p * len(argv))(*argv)).decode().splitlines():
        k, v = line.split("=", 1)
        if k == "note":
            o["notes"].append(v)
        else:
            o[k] = v
    return o


def test_defaults_are_the_references(lib):
    o = parse(lib, "-i", "x.mvs")
    assert int(o["result"]) == OK and o["depthPriors"] == "" and (float(o["paraPrior"]), float(o["sigmaPrior"]), int(o["photo2geo"])) == (0.5, 0.2, 2)


def test_the_options_parse(lib):
    o = parse(lib, "-i", "x.mvs", "--depth-priors", "/data/priors", "--n-para_prior", "0.4", "--sigma-prior=0.25", "--n-photo2geo", "1")
    assert int(o["result"]) == OK and o["depthPriors"] == "/data/priors"
    assert (float(o["paraPrior"]), float(o["sigmaPrior"]), int(o["photo2geo"])) == (pytest.approx(0.4), 0.25, 1)
    # the authors' command line: the three options without a folder are read and change nothing
    o = parse(lib, "-i", "x.mvs", "--use-semantic", "1", "--n-para_prior", "0.4", "--n-photo2geo", "1")
    assert int(o["result"]) == OK and o["depthPriors"] == ""
    assert o["notes"] == ["--use-semantic is not available in this build (defined subset); treated as 0 (prior depth maps made elsewhere can be supplied with "
                          "--depth-priors <folder>)"]
    assert parse(lib, "-i", "x.mvs", "--sigma-prior", "0")["result"] == "0"     # ... not even a value the term could not use


def test_the_exclusive_combinations_are_errors(lib):
    for extra, word in ((["--restore-hypothesis", "1"], "--restore-hypothesis"), (["--n-viewspread", "1"], "--n-viewspread")):
        o = parse(lib, "-i", "x.mvs", "--depth-priors", "p", *extra)
        assert int(o["result"]) == ERROR and word in o["err"] and "--depth-priors" in o["err"]
        assert int(parse(lib, "-i", "x.mvs", *extra)["result"]) == OK
        assert int(parse(lib, "-i", "x.mvs", "--depth-priors", "p", extra[0], "0")["result"]) == OK
    for extra, word in ((["--n-para_prior", "1.5"], "--n-para_prior"), (["--n-para_prior", "-0.1"], "--n-para_prior"), (["--sigma-prior", "0"], "--sigma-prior"),
                        (["--sigma-prior", "-1"], "--sigma-prior"), (["--n-photo2geo", "-1"], "--n-photo2geo")):
        o = parse(lib, "-i", "x.mvs", "--depth-priors", "p", *extra)
        assert int(o["result"]) == ERROR and word in o["err"]


def test_the_schedule_follows_the_reference(lib):
    out = (C.c_int * 2)()
    for n_ext in (1, 2, 3, 4):
        for it in range(n_ext):
            lib.dq_schedule(b"p", n_ext, it, out)
            assert (out[0], out[1]) == (int(it == n_ext - 2), int(n_ext < 2))
            lib.dq_schedule(b"", n_ext, it, out)
            assert (out[0], out[1]) == (0, 0)
    assert lib.dq_path(b"/data/priors", 7).decode() == "/data/priors/depth0007.prior.dmap"
