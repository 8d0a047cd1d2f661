"""distributed.densify_scene(plane_priors=...): the priors generated on the device from the live maps on outer iteration n - 2 give, bit for
bit, what densify_scene(priors=<the maps it returned>) gives -- from the generation on, the path is that of priors=."""
import importlib

import numpy as np
import pytest

import test_gpu_driver_spread as DS
import test_gpu_schedule as GS

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")
D = importlib.import_module("hc-mvs_amd.distributed")

SEED, OUTER = 779, 2
KW = dict(adapthalfwin=6, n_estimation_iters=2, propagate_halfwin=5, propagate_step=4, photometric_flow=0.0)
PRIOR = dict(para_prior=0.4, sigma_prior=0.2, photo2geo=1)


def test_generated_priors_equal_the_same_maps_given_as_priors(tmp_path):
    import torch
    views, verts, _ = GS._driver_scene(str(tmp_path), n=4, w=128, h=96)
    oviews, srcs, neighbors, order, init = DS._oracle_inputs(views, verts)
    labels = np.zeros((96, 128), np.uint16); labels[10:86, 12:116] = 255
    half = np.zeros((48, 64), np.uint16); half[:, 20:] = 9          # another size, another label
    plane_priors = {0: labels, 2: labels, 3: half}
    ctx = binding.Context(0)
    try:
        p = binding.default_params(seed=SEED, **KW)
        dev = torch.device("cuda", 0)
        run = lambda **kw: D.densify_scene(ctx, oviews, srcs, neighbors, order, init, p, device=dev, n_external_iters=OUTER, prior_params=PRIOR, **kw)
        ppp = binding.default_plane_prior_params(seed=5)
        a = run(plane_priors={0: labels, 2: labels}, plane_prior_params=ppp)
        assert a["priors_used"] is True and sorted(a["plane_prior_maps"]) == [0, 2]
        maps = {i: m.cpu().numpy() for i, m in a["plane_prior_maps"].items()}
        print("planes", a["plane_prior_planes"], "prior pixels", {i: int((m > 0).sum()) for i, m in maps.items()})
        assert all(a["plane_prior_planes"][i] >= 1 and (maps[i] > 0).sum() > 1000 and not maps[i][labels != 255].any() for i in maps)
        assert not ctx.get_prior_region(0).any()                        # the call's regions are gone with it
        b = run(priors=maps)
        for i in order:
            for x, y, what in zip(a["maps"][i], b["maps"][i], ("depth", "normal", "conf")):
                assert torch.equal(x, y), "%s map %d" % (what, i)
        assert a["n_points"] == b["n_points"] > 1000 and np.array_equal(a["xyz"], b["xyz"])
        plain = run()
        assert any(not torch.equal(a["maps"][i][0], plain["maps"][i][0]) for i in (0, 2))       # the priors were at work
        # the label of the parameters decides the region: label 9 of the smaller image
        c = run(plane_priors={3: half}, plane_prior_params=binding.default_plane_prior_params(region_label=9), fuse=False)
        m3 = c["plane_prior_maps"][3].cpu().numpy()
        assert not m3[:, :40].any()
        # fewer than two outer iterations: nothing is generated, which is noted, not raised
        one = D.densify_scene(ctx, oviews, srcs, neighbors, order, init, p, device=dev, n_external_iters=1, plane_priors=plane_priors, fuse=False)
        assert one["priors_used"] is False and one["plane_prior_maps"] == {}
        with pytest.raises(ValueError, match="priors and in plane_priors"):
            run(plane_priors={0: labels}, priors={0: maps[0]})
        with pytest.raises(ValueError):
            run(plane_priors={0: labels}, viewspread=True)
    finally:
        ctx.close()
