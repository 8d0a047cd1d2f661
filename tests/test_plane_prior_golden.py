"""The numpy statement of the plane-prior rule (tests/plane_prior_ref.py) against tests/golden/plane_prior_statement.json: what the two
statements this repository had before they were folded into one returned -- the rule without S4c ("unclustered") and its copy with S4c
("clustered", at cluster_mul 0 too) -- item by item and exactly.  tests/golden/make_golden_plane_prior.py says how a call is recorded."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_plane_prior as G  # noqa: E402
import plane_prior_cases as cases  # noqa: E402
import plane_prior_ref as ref  # noqa: E402
import test_plane_prior_ref as TR  # noqa: E402

with open(G.PATH) as f:
    RECORDED = json.load(f)


def test_the_file_holds_the_calls_the_generator_lists():
    assert [(r["source"], r["case"], r["params"]) for r in RECORDED] == [(s, n, p) for s, n, p in G.calls(cases.CASES, cases.CLUSTER_CASES)]
    assert len(RECORDED) == 8 + 16 + 28 + 2 + 3


@pytest.mark.parametrize("rec", RECORDED, ids=["%s-%s-%s" % (r["source"], r["case"], "-".join("%s=%s" % kv for kv in r["params"].items())) for r in RECORDED])
def test_the_statement_returns_the_recorded_bits(rec):
    c, state = TR.stages(rec["case"])
    got = ref.generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], state=state, **rec["params"])
    enc = G.encode(rec["source"], got)
    for part in ("arrays", "stats"):
        assert set(enc[part]) == set(rec[part])
        for k, v in rec[part].items():
            assert enc[part][k] == v and type(enc[part][k]) is type(v), (part, k)
    assert enc["planes"] == rec["planes"]
    if rec["source"] == "unclustered":                   # what the one statement adds to a call without S4c
        win = got["rounds"][:, 0] >= 0
        assert got["clusters"].dtype == np.int32 and got["clusters"].shape == (len(got["rounds"]), 4) and not got["clusters"][~win].any()
        assert np.array_equal(got["clusters"][win], [[0, 0, n, 1] for n in got["rounds"][win, 1]])
        st = got["stats"]
        assert st["cluster_eps"] == 0 and type(st["cluster_eps"]) is np.float32 and st["cluster_rejects"] == 0 and st["cluster_left"] == 0
