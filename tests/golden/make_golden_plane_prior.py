"""Generates tests/golden/plane_prior_statement.json: what the numpy statement of the plane-prior rule (tests/plane_prior_ref.py) returns,
held by tests/test_plane_prior_golden.py.  The committed file was recorded with the two statements this repository had before they were
folded into one -- plane_prior_ref.generate without S4c ("unclustered") and the copy of it with S4c ("clustered") --, through record()
below with those two functions and the two dicts of cases; run on the folded statement this generator reproduces it byte for byte.
Regenerate only when the rule changes on purpose.
Run from the repo root: python tests/golden/make_golden_plane_prior.py

A call is recorded as one SHA-256 per array (over dtype, shape and bytes), one per plane (over normal, centre, quad and nc), and in clear a
plane's n_inliers and box_fallback and every stat: an int as it is, a double as float.hex(), a float32 as "f32:" + float.hex().  An
unclustered call records what the statement without S4c returned: neither `clusters` nor the cluster_* stats."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "plane_prior_statement.json")
ARRAYS = ("prior", "prior_normal", "stage", "assignment", "rounds", "clusters")
SEEDS = (1, 2)
CLUSTERED_TOO = ("crease", "two_blobs", "plane_and_sphere")       # the cases of CASES that are also recorded with S4c at work


def calls(cases, cluster_cases):
    """(source, case, parameters) of every recorded call, in the file's order"""
    out = [("unclustered", name, dict(seed=s)) for name in cases for s in SEEDS]
    out += [("clustered", name, dict(seed=s, cluster_mul=0.0)) for name in list(cases) + list(cluster_cases) for s in SEEDS]
    out += [("clustered", name, dict(seed=s, cluster_mul=mul)) for name in list(cluster_cases) + list(CLUSTERED_TOO) for s in SEEDS for mul in (2.0, 3.0)]
    out += [("clustered", "islands", dict(seed=s, cluster_mul=2.0, min_points_div=4.0)) for s in SEEDS]
    out += [("clustered", "doorway", dict(seed=1, cluster_mul=mul)) for mul in (40.0, 1e-9, 1e-45)]
    return out


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s %s " % (a.dtype.str, a.shape)).encode()); h.update(a.tobytes())
    return h.hexdigest()


def stat(v):
    if type(v) is np.float32:
        return "f32:" + float(v).hex()
    if type(v) in (float, np.float64):
        return float(v).hex()
    assert type(v) in (int, np.int64), type(v)
    return int(v)


def encode(source, res):
    """the recorded form of what a generate() returned"""
    plain = source == "unclustered"
    arrays = {k: digest(res[k]) for k in ARRAYS if not (plain and k == "clusters")}
    arrays["flags.S2"] = digest(res["flags"]["S2"])
    planes = [dict(sha256=digest(p["normal"], p["centre"], p["quad"], p["nc"]), n_inliers=int(p["n_inliers"]), box_fallback=int(p["box_fallback"]))
              for p in res["planes"]]
    stats = {k: stat(v) for k, v in res["stats"].items() if not (plain and k.startswith("cluster_"))}
    return dict(arrays=arrays, planes=planes, stats=stats)


def record(generate, fitting_set, cases, cluster_cases):
    """generate: dict source -> the statement's generate; returns the list of recorded calls"""
    made, out = {}, []
    for source, name, params in calls(cases, cluster_cases):
        if name not in made:
            c = (cases[name] if name in cases else cluster_cases[name])()
            made[name] = (c, fitting_set(c["depth"], c["normal"], c["conf"], c["region"], c["K"]))
        c, state = made[name]                    # S1 .. S3 read none of the parameters that vary here
        res = generate[source](c["depth"], c["normal"], c["conf"], c["region"], c["K"], state=state, **params)
        out.append(dict(source=source, case=name, params=params, **encode(source, res)))
        print("%-11s %-16s %-60s planes %d rounds %d" % (source, name, params, len(res["planes"]), len(res["rounds"])))
    return out


def write(recorded):
    with open(PATH, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in recorded) + "\n]\n")
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE))); sys.path.insert(0, os.path.dirname(HERE))
    import plane_prior_cases as cases
    import plane_prior_ref as ref
    write(record(dict(unclustered=ref.generate, clustered=ref.generate), ref.fitting_set, cases.CASES, cases.CLUSTER_CASES))
