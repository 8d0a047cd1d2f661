"""Generates tests/golden/plane_prior_refit_statement.json: what the statement of the plane-prior rule with the refit of a round's winner
(tests/plane_prior_refit_ref.py) returns, held by tests/test_plane_prior_refit_ref.py.  Regenerate only when
the rule changes on purpose.
Run from the repo root: python tests/golden/make_golden_plane_prior_refit.py

A call is recorded as make_golden_plane_prior.py records one (a SHA-256 per array and per plane, the stats in clear), with the arrays
`refits` and `refit_planes` among them, the reason every round's steps ended in clear, and every step solved in clear: the number of band
samples, the nine integer sums, the anchor and the two planes as float.hex() -- what the solver of prior_gen_plan.h is compared on
(tests/test_prior_refit_plan.py)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_plane_prior as G  # noqa: E402

PATH = os.path.join(HERE, "plane_prior_refit_statement.json")
ARRAYS = G.ARRAYS + ("refits", "refit_planes")
SEEDS = (1, 2)
# the inputs on which the steps end for each of the reasons: the tiny eps makes planes of a few samples (band, count and fixed point, and
# the saturation of the moments: E = -20); min_points right at the winner's cnt_0 makes the first step of the crease lose the count
STOP_CALLS = (("two_blobs", dict(seed=1, refit_iters=4, epsilon_mul=1e-5, min_points_div=1e6, max_rounds=6)),
              ("crease", dict(seed=3, refit_iters=4, min_points_div=1.86)))


def calls(cases):
    """(case, parameters) of every recorded call, in the file's order"""
    out = [(name, dict(seed=s, refit_iters=r)) for name in cases for s in SEEDS for r in (1, 4)]
    out += [("doorway", dict(seed=s, refit_iters=4, cluster_mul=2.0)) for s in SEEDS]
    out += [(name, dict(p)) for name, p in STOP_CALLS]
    return out


def encode(res):
    arrays = {k: G.digest(res[k]) for k in ARRAYS}
    arrays["flags.S2"] = G.digest(res["flags"]["S2"])
    planes = [dict(sha256=G.digest(p["normal"], p["centre"], p["quad"], p["nc"]), n_inliers=int(p["n_inliers"]), box_fallback=int(p["box_fallback"]))
              for p in res["planes"]]
    stats = {k: G.stat(v) for k, v in res["stats"].items()}
    steps = [dict(m=int(s["m"]), sums=[int(v) for v in s["sums"]], O=[float(v).hex() for v in s["O"]], E=int(s["E"]), prev=[float(v).hex() for v in s["prev"]],
                  plane=[float(v).hex() for v in s["plane"]]) for s in res["refit_cov"]]
    return dict(arrays=arrays, planes=planes, stats=stats, stops=list(res["refit_stops"]), steps=steps)


def record(generate, fitting_set, cases, cluster_cases):
    made, out = {}, []
    for name, params in calls(cases):
        if name not in made:
            c = (cases[name] if name in cases else cluster_cases[name])()
            made[name] = (c, fitting_set(c["depth"], c["normal"], c["conf"], c["region"], c["K"]))
        c, state = made[name]                    # S1 .. S3 read none of the parameters that vary here
        res = generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], state=state, **params)
        out.append(dict(case=name, params=params, **encode(res)))
        print("%-16s %-90s planes %d rounds %d steps %d %s" % (name, params, len(res["planes"]), len(res["rounds"]), res["stats"]["refit_steps"], res["refit_stops"]))
    return out


def write(recorded):
    with open(PATH, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in recorded) + "\n]\n")
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE))); sys.path.insert(0, os.path.dirname(HERE))
    import plane_prior_cases as cases
    import plane_prior_ref as ref
    import plane_prior_refit_ref as refit
    write(record(refit.generate, ref.fitting_set, cases.CASES, cases.CLUSTER_CASES))
