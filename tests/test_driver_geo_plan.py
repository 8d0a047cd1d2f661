"""The geometric-consistency options of the driver's plan (hc-mvs_amd/host/driver_plan.h) on the CPU: --geo-consistency and --geo-max-px,
fed by --n-para_tapa, --n-para_tapa2, --n-txthreshold, --n-txthreshold2 and --n-photo2geo; the refused combinations are parse errors;
--n-usegeoconsistency keeps its note word for word; the source views' maps are offered on the iterations view spread offers them.
tests/driver_geo_shim.cpp is compiled with g++ alone: no HIP, no library."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "driver_geo_shim.cpp")
HOST = os.path.join(ROOT, "hc-mvs_amd", "host")
HDRS = [os.path.join(HOST, "driver_plan.h"), os.path.join(HOST, "scene_io.h"), os.path.join(ROOT, "include", "hcmvs_hip.h")]
LIB_PATH = os.path.join(HERE, "libdriver_geo_shim.so")
OK, USAGE, ERROR = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in [SRC] + HDRS):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    L.dg_parse.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    L.dg_parse.restype = C.c_char_p
    L.dg_iteration.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)]
    L.dg_iteration.restype = None
    L.dg_usage.restype = C.c_char_p
    return L


def parse(lib, *args):
    argv = [b"DensifyPointCloud"] + [a.encode() for a in args]
    o = dict(notes=[])
    for line in lib.dg_parse(len(argv), (C.c_char_p * len(argv))(*argv)).decode().splitlines():
        k, v = line.split("=", 1)
        if k == "note":
            o["notes"].append(v)
        else:
            o[k] = v
    return o


def values(o):
    return (int(o["on"]), float(o["para_tapa"]), float(o["para_tapa2"]), float(o["txthreshold"]), float(o["txthreshold2"]), int(o["photo2geo"]), float(o["max_px"]))


def test_defaults(lib):
    o = parse(lib, "-i", "x.mvs")
    assert int(o["result"]) == OK and values(o) == (0, 0.25, pytest.approx(0.15), 150.0, 160.0, 2, 3.0)


def test_the_feeding_options(lib):
    o = parse(lib, "-i", "x.mvs", "--geo-consistency", "1", "--n-para_tapa", "0.26", "--n-para_tapa2=0.26", "--n-txthreshold", "120", "--n-txthreshold2", "140",
              "--n-photo2geo", "1", "--geo-max-px", "2.5")
    assert int(o["result"]) == OK and values(o) == (1, pytest.approx(0.26), pytest.approx(0.26), 120.0, 140.0, 1, 2.5)
    # the authors' command line: the fork's switch keeps its note word for word, the feeding options are read and change nothing
    o = parse(lib, "-i", "x.mvs", "-v", "2", "--n-usegeoconsistency", "1", "--n-para_tapa", "0.26", "--n-photo2geo", "1")
    assert int(o["result"]) == OK and int(o["on"]) == 0
    assert o["notes"] == ["--n-usegeoconsistency is not available in this build (defined subset); treated as 0"]
    assert parse(lib, "-i", "x.mvs", "--n-para_tapa", "7")["result"] == "0"         # ... not even a value the term could not use
    assert b"--geo-consistency 0|1" in lib.dg_usage() and b"--geo-max-px" in lib.dg_usage()


@pytest.mark.parametrize("extra,word", [(("--n-viewspread", "1"), "--n-viewspread 1"), (("--restore-hypothesis", "1"), "--restore-hypothesis 1"),
                                        (("--depth-priors", "/p"), "--depth-priors"), (("--plane-priors", "1"), "--plane-priors 1")])
def test_each_refused_combination_is_a_parse_error(lib, extra, word):
    o = parse(lib, "-i", "x.mvs", "--geo-consistency", "1", *extra)
    assert int(o["result"]) == ERROR and "--geo-consistency 1 is not combined with " + word in o["err"]
    assert int(parse(lib, "-i", "x.mvs", "--geo-consistency", "0", *extra)["result"]) == OK


def test_values_the_term_cannot_use(lib):
    for args in (("--geo-consistency", "2"), ("--geo-consistency", "1", "--n-para_tapa", "1.5"), ("--geo-consistency", "1", "--n-para_tapa2", "-0.1"),
                 ("--geo-consistency", "1", "--n-txthreshold", "inf"), ("--geo-consistency", "1", "--geo-max-px", "0"), ("--geo-consistency", "1", "--n-photo2geo", "-1")):
        assert int(parse(lib, "-i", "x.mvs", *args)["result"]) == ERROR, args
    assert int(parse(lib, "-i", "x.mvs", "--geo-max-px")["result"]) == ERROR       # the value is missing


def test_the_maps_are_offered_as_for_view_spread(lib):
    out = (C.c_int * 3)()
    for it, want in ((0, (0, 0, 0)), (1, (1, 0, 0)), (2, (1, 0, 0))):
        lib.dg_iteration(1, 0, 3, it, out)
        assert tuple(out[:]) == want
    lib.dg_iteration(1, 1, 3, 1, out)
    assert tuple(out[:]) == (0, 1, 1)                  # the interleaved schedule offers the live maps
    lib.dg_iteration(0, 0, 3, 1, out)
    assert tuple(out[:]) == (0, 0, 0)
