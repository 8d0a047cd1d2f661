"""The host side of the view selection without a GPU: hcmvs_default_view_select_params gives the reference's defaults, and
distributed.plan_scene orders the selected images as the driver's plan_deal does (best connected first, stable)."""
import ctypes as C
import importlib

import pytest

binding = importlib.import_module("hc-mvs_amd.binding")
D = importlib.import_module("hc-mvs_amd.distributed")


def test_default_view_select_params_are_the_reference_defaults():
    p = binding.ViewSelectParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    binding.lib().hcmvs_default_view_select_params(C.byref(p))
    # OPTDENSE::nMinViews, nMinViewsTrustPoint > 1 ? it : 2, nMaxViews, --number-views (DepthMap.cpp:72-86, SceneDensify.cpp:313)
    assert (p.n_min_views, p.n_min_point_views, p.n_max_views, p.number_views) == (2, 2, 12, 5)
    assert (p.optim_angle_deg, p.min_angle_deg, p.max_angle_deg) == (10.0, 3.0, 65.0)
    assert p.min_area == pytest.approx(0.01, rel=1e-7) and p.min_scale == pytest.approx(0.2, rel=1e-7) and p.max_scale == pytest.approx(3.2, rel=1e-7)
    assert p.min_score_ratio == pytest.approx(0.3, rel=1e-7) and p.min_score == 0.0
    assert C.sizeof(p) == 48
    q = binding.default_view_select_params(number_views=0, n_max_views=64)
    assert (q.number_views, q.n_max_views, q.n_min_views) == (0, 64, 2)
    with pytest.raises(AttributeError):
        binding.default_view_select_params(no_such_field=1)
    binding.lib().hcmvs_default_view_select_params(None)  # a null pointer is ignored


def test_plan_order_is_by_decreasing_neighbour_count_and_stable():
    counts = {0: 3, 1: 5, 2: 3, 4: 5, 7: 1, 9: 3}
    assert D.plan_order([0, 1, 2, 4, 7, 9], counts) == [1, 4, 0, 2, 9, 7]
    assert D.plan_order([9, 7, 4, 2, 1, 0], counts) == [4, 1, 9, 2, 0, 7]     # ties keep the order given
    assert D.plan_order([], counts) == []
    assert D.plan_order(range(3), [2, 2, 2]) == [0, 1, 2]


class FakeContext:
    """select_views as binding.Context returns it, for plan_scene's bookkeeping"""

    def __init__(self, result):
        self.result, self.args = result, None

    def select_views(self, *a, **kw):
        self.args = (a, kw)
        return self.result


def test_plan_scene_shapes_what_densify_scene_takes():
    def image(ids, n_src, points):
        return dict(points=points, neighbors=[dict(id=i, points=9, scale=1.0, angle=0.2, area=0.5, score=9.0 - k) for k, i in enumerate(ids)],
                    srcs=[(i, 1.0 if k else 1.3) for k, i in enumerate(ids[:n_src])], avg_depth=5.0, status=0)

    ctx = FakeContext([image([1, 3], 2, [0, 2, 5, 6]), image([0, 3, 4], 2, [1, 2, 3, 4]), None, image([1, 0, 4], 3, [4, 5, 6, 7]), image([3, 1], 1, [0, 1, 2, 7])])
    srcs, neighbors, order, points = D.plan_scene(ctx, "cams", "sizes", "xyz", "nv", "ids", number_views=3, n_max_views=9)
    assert ctx.args == (("cams", "sizes", "xyz", "nv", "ids"), dict(number_views=3, n_max_views=9))
    assert srcs == {0: [1, 3], 1: [0, 3], 3: [1, 0, 4], 4: [3]}
    assert neighbors == {0: [1, 3], 1: [0, 3, 4], 3: [1, 0, 4], 4: [3, 1]}
    assert order == [1, 3, 0, 4]                                              # 3, 3, 2, 2 neighbours; image 2 got no views
    assert sorted(points) == [0, 1, 3, 4] and list(points[3]) == [4, 5, 6, 7]
