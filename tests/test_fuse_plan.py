"""The host-side plans of the fusion and of the post-filter chain (hc-mvs_amd/csrc/fuse_plan.h) on the CPU: the dimensions of a fusion call
and their limits, the layout of the per-pass tables, the layout of the chain's state.  tests/fuse_plan_shim.cpp is compiled with g++ alone:
no HIP, no library.  Arithmetic only, nothing is allocated.

The expected totals are a transcription of the carve statements the entry points had before the plans existed (every piece rounded up to
256 bytes on its own); the sizes a piece needs are those the kernel side documents in fuse_common.h and pf_chain.h."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "fuse_plan_shim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "hc-mvs_amd", "csrc")
HDRS = [os.path.join(CSRC, "fuse_plan.h"), os.path.join(CSRC, "carve.h")]
LIB_PATH = os.path.join(HERE, "libfuse_plan_shim.so")
U64 = C.c_ulonglong
U32 = C.c_uint32

OK, NO_MAPS, TOO_MANY_NEIGHBORS, STRIDE_LIMIT, TABLE_LIMIT = range(5)   # FuseLimit
CTL = 256        # kCtlBytes
PF_IMAGE = 104   # stands in for sizeof(PfImage)
AREAS = (1, 255, 256, 257, 96 * 80)
NEIGHBORS = (0, 1, 3, 31)
CORE = ("pending", "settle", "targets", "head", "next", "ctl", "counters", "status", "merged", "flag", "nv")
CLOUD_TAIL = ("totals", "flag32", "pos", "scan", "xyz", "nrm", "bgr", "pviews", "pweights", "voff")
CHAIN_IMAGE = ("own", "chgNow", "valNext", "tgt", "head", "next", "acc", "mm", "fm", "stamp", "touch", "stride", "inOrder")
CHAIN_TAIL = ("anyChg", "table", "scratch", "ctl", "counters", "status", "dF", "dF2", "nF")


def r256(b):
    return (b + 255) & ~255


def settle_bytes(p):      # fuse_settle_bytes (fuse_kernels.hip): three word lists and one byte per pixel
    return r256(p * 4) * 3 + p


def pf_scratch_bytes(p):  # pf_pass_scratch_bytes (pf_kernels.hip)
    return r256(p * 4) * 6 + r256(p)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in [SRC] + HDRS):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    table = [P(U64), P(C.c_int), P(C.c_int), P(U32), C.c_int]
    L.fup_max_views.restype = C.c_int
    L.fup_dims.argtypes = table + [P(U32), C.c_int, P(U64)]
    L.fup_dims.restype = None
    L.fup_cloud_pass.argtypes = [U64, U64, C.c_int, U64, U64, U64, C.c_int, P(U64)]
    L.fup_cloud_pass.restype = U64
    L.fup_postfilter_pass.argtypes = [U64, U64, C.c_int, U64, U64, U64, P(U64)]
    L.fup_postfilter_pass.restype = U64
    L.fup_cloud_out.argtypes = [U64, U64, C.c_int, C.c_int, C.c_int, C.c_int, P(U64)]
    L.fup_cloud_out.restype = U64
    L.fup_chain.argtypes = table + [P(U32), C.c_int, P(U32), C.c_int, U64, U64, U64, U64, P(U64), P(U64), P(U64)]
    L.fup_chain.restype = C.c_int
    return L


class Img:
    def __init__(self, pixels, nbs=(), maps=True):
        self.pixels, self.nbs, self.maps = pixels, list(nbs), maps


def table_args(scene):
    n = len(scene)
    first = [0]
    for m in scene:
        first.append(first[-1] + len(m.nbs))
    flat = [nb for m in scene for nb in m.nbs]
    return ((U64 * max(n, 1))(*[m.pixels for m in scene]), (C.c_int * max(n, 1))(*[int(m.maps) for m in scene]), (C.c_int * (n + 1))(*first),
            (U32 * max(len(flat), 1))(*flat), n)


def u32s(v):
    return (U32 * max(len(v), 1))(*v)


def dims(lib, scene, order):
    out = (U64 * 5)()
    lib.fup_dims(*table_args(scene), u32s(order), len(order), out)
    at = out[4] if out[4] < 2 ** 63 else out[4] - 2 ** 64
    return dict(maxArea=out[0], stride=out[1], maxNb=out[2], broken=out[3], at=at)


def chain(lib, scene, ids, order, max_id_area=None, scratch=None):
    in_order = [scene[i].pixels for i in order if i < len(scene) and scene[i].maps]
    if max_id_area is None:
        max_id_area = max(scene[i].pixels for i in ids)
    if scratch is None:
        scratch = pf_scratch_bytes(max(in_order, default=0))
    img = (U64 * (13 * max(len(scene), 1)))(); tail = (U64 * 9)(); total = U64()
    ok = lib.fup_chain(*table_args(scene), u32s(ids), len(ids), u32s(order), len(order), max_id_area, PF_IMAGE, scratch, CTL, img, tail, C.byref(total))
    if not ok:
        return None
    images = [dict(zip(CHAIN_IMAGE, img[13 * i:13 * i + 13])) for i in range(len(scene))]
    return dict(images=images, tail=dict(zip(CHAIN_TAIL, tail)), bytes=total.value)


def check_layout(pieces, total):
    """pieces: (name, offset, bytes its user needs).  256-aligned, none overlaps another, all inside the allocation"""
    used = sorted((off, need, name) for name, off, need in pieces)
    for off, need, name in used:
        assert off % 256 == 0, name
    for (off, need, name), (nxt, _, other) in zip(used, used[1:]):
        assert off + need <= nxt, (name, other)
    assert used[-1][0] + used[-1][1] <= total, used[-1][2]


def core_needs(area, stride, nb):
    """per-pass tables of image A (fuse_common.h FuseTables, launch_fuse_begin / launch_fuse_pass), for the largest image and neighbour count"""
    return dict(pending=area * 4,          # the pending pixels: at most every pixel, a word each
                settle=settle_bytes(area),
                targets=area * nb * 4,     # [w*h][nNeighbors] int32
                head=nb * stride * 4,      # [nNeighbors][stride] uint32
                next=nb * area * 4,        # [nNeighbors][w*h] uint32
                ctl=CTL, counters=6 * 8,   # counters[0 .. 5]
                status=4 * 4,              # status[0 .. 3]
                merged=area * 4, flag=area, nv=area * 4)


# ---- totals: what each entry point reserves is what it reserved before the plan existed ----

def test_fusion_dimensions_of_small_scenes(lib):
    assert lib.fup_max_views() == 32
    for area, nb, larger in itertools.product(AREAS, NEIGHBORS, (0, 1000)):
        # image 0 is fused; its neighbours are images 1 .. (image 1 has maps, possibly larger ones; the rest do not exist); image 40 has maps too
        scene = [Img(area, nbs=range(1, nb + 1)), Img(area + larger)] + [Img(0, maps=False)] * 38 + [Img(7)]
        d = dims(lib, scene, [0])
        assert d == dict(maxArea=area, stride=max(area + larger, 7), maxNb=max(nb, 1), broken=OK, at=-1)
    d = dims(lib, [Img(300, nbs=[1, 2]), Img(200, nbs=[0, 2, 0]), Img(100)], [1, 0, 2])
    assert d == dict(maxArea=300, stride=300, maxNb=3, broken=OK, at=-1)


def test_cloud_pass_reserves_what_hcmvs_fuse_cloud_reserved(lib):
    for area, nb, larger, lists, scan in itertools.product(AREAS, NEIGHBORS, (0, 1000), (False, True), (256, 7 * 256)):
        max_nb, stride = max(nb, 1), area + larger
        off = (U64 * 21)()
        total = lib.fup_cloud_pass(area, stride, max_nb, settle_bytes(area), CTL, scan, int(lists), off)
        per_view = area * 4 * (max_nb + 1) if lists else 0
        parent = [area * 4, settle_bytes(area), area * 4 * max_nb, stride * max_nb * 4, area * 4 * max_nb, CTL, 64, 64, 64,
                  area * 4, area, area * 4, area * 4, scan, area * 12, area * 12, area * 3, area * 4, per_view, per_view, area * 4 if lists else 0]
        assert total == sum(r256(b) for b in parent), (area, nb, larger, lists, scan)
        need = core_needs(area, stride, max_nb)
        need.update(totals=3 * 8, flag32=area * 4, pos=area * 4, scan=scan, xyz=area * 12, nrm=area * 12, bgr=area * 3,
                    pviews=per_view, pweights=per_view,     # [w*h][vstride = maxNb + 1] ids / weights of a point's views
                    voff=area * 4 if lists else 0)
        names = CORE + CLOUD_TAIL
        check_layout([(k, off[i], need[k]) for i, k in enumerate(names)], total)


def test_postfilter_pass_reserves_what_hcmvs_postfilter_sequence_reserved(lib):
    for area, nb, larger, id_area in itertools.product(AREAS, NEIGHBORS, (0, 1000), (1, 257, 96 * 80, 640 * 480)):
        max_nb, stride = max(nb, 1), area + larger
        off = (U64 * 14)()
        total = lib.fup_postfilter_pass(area, stride, max_nb, settle_bytes(area), CTL, id_area, off)
        parent = [area * 4, settle_bytes(area), area * 4 * max_nb, stride * max_nb * 4, area * 4 * max_nb, CTL, 64, 64, area * 4, area, area * 4,
                  id_area * 4, id_area * 4, id_area * 12]
        assert total == sum(r256(b) for b in parent), (area, nb, larger, id_area)
        need = core_needs(area, stride, max_nb)
        need.update(dF=id_area * 4, dF2=id_area * 4, nF=id_area * 12)   # launch_postfilter: w*h floats each, 3*w*h floats
        names = CORE + ("dF", "dF2", "nF")
        check_layout([(k, off[i], need[k]) for i, k in enumerate(names)], total)
        # the post-filter reserves no cloud-only piece: nothing beyond the core and its own three
        assert total == sum(r256(need[k]) for k in names)


def test_cloud_copy_reserves_what_hcmvs_fuse_cloud_reserved(lib):
    for cap, vcap, xyz, nrm, bgr, nv in itertools.product((0, 1, 1000, 96 * 80 * 3), (0, 5000), *[(0, 1)] * 4):
        off = (U64 * 6)()
        total = lib.fup_cloud_out(cap, vcap, xyz, nrm, bgr, nv, off)
        need = [cap * 12 if xyz else 0, cap * 12 if nrm else 0, cap * 3 if bgr else 0, cap * 4 if nv or vcap else 0, vcap * 4, vcap * 4]
        assert total == max(sum(r256(b) for b in need), 256), (cap, vcap, xyz, nrm, bgr, nv)
        check_layout(list(zip(("xyz", "normal", "bgr", "nViews", "viewIds", "viewWeights"), off, need)), total)


def chain_scene(area, nb, larger):
    """images 0 .. 2 are fused (0 with nb neighbours, one of them larger), 3 and 4 have maps but are not fused, 5 is a view without maps, 6 no view
    at all, 7 a neighbour that no longer has maps"""
    return [Img(area, nbs=list(range(1, nb + 1))), Img(area + larger, nbs=[0, 3, 7]), Img(257, nbs=[6, 5]), Img(area + 3), Img(12, nbs=[0]),
            Img(50, maps=False), Img(0, maps=False), Img(10 ** 6, nbs=[0], maps=False)] + [Img(0, maps=False)] * 24


def parent_chain_bytes(scene, ids, order):
    total, max_area = 0, 0
    for i, m in enumerate(scene):
        if not m.maps:
            continue
        n = m.pixels
        total += r256(n * 2) + r256(n) + r256(n)
        if i not in order:
            continue
        stride = max([1] + [scene[nb].pixels for nb in m.nbs if nb < len(scene) and scene[nb].maps])
        nnb = max(len(m.nbs), 1)
        total += r256(n * nnb * 4) + r256(nnb * stride * 4) + r256(2 * nnb * n * 4) + r256(n) + 4 * r256(n * 4)
        max_area = max(max_area, n)
    max_id = max(scene[i].pixels for i in ids)
    return total + r256(len(scene) * 4) + r256(len(scene) * PF_IMAGE) + r256(pf_scratch_bytes(max_area)) + r256(CTL) + 2 * r256(64) + 2 * r256(max_id * 4) + r256(max_id * 12)


def test_chain_state_reserves_what_the_chain_reserved(lib):
    for area, nb, larger in itertools.product(AREAS, NEIGHBORS, (0, 1000)):
        scene = chain_scene(area, nb, larger)
        ids, order = [3, 0, 4], [2, 0, 1]
        p = chain(lib, scene, ids, order)
        assert p is not None and p["bytes"] == parent_chain_bytes(scene, ids, order), (area, nb, larger)
        pieces = []
        for i, (m, L) in enumerate(zip(scene, p["images"])):
            assert L["inOrder"] == (i in order)
            if not m.maps:
                assert not any(L[k] for k in CHAIN_IMAGE[:12]), i   # an id without maps takes no room
                continue
            n = m.pixels
            pieces += [("own%d" % i, L["own"], n * 2), ("chgNow%d" % i, L["chgNow"], n), ("valNext%d" % i, L["valNext"], n)]   # pf_chain.h: u16, u8, u8 per pixel
            if i not in order:
                continue
            nnb = max(len(m.nbs), 1)
            stride = max([1] + [scene[q].pixels for q in m.nbs if q < len(scene) and scene[q].maps])
            assert L["stride"] == stride
            pieces += [("tgt%d" % i, L["tgt"], n * nnb * 4),           # [w*h][nNeighbors]
                       ("head%d" % i, L["head"], nnb * stride * 4),   # [nNeighbors][stride]
                       ("next%d" % i, L["next"], 2 * nnb * n * 4),    # [2][nNeighbors][w*h]
                       ("acc%d" % i, L["acc"], n)] + [("%s%d" % (k, i), L[k], n * 4) for k in ("mm", "fm", "stamp", "touch")]
        t = p["tail"]
        max_id = max(scene[i].pixels for i in ids)
        tail_need = dict(anyChg=len(scene) * 4, table=len(scene) * PF_IMAGE, scratch=pf_scratch_bytes(max(scene[i].pixels for i in order)), ctl=CTL,
                         counters=6 * 8, status=4 * 4, dF=max_id * 4, dF2=max_id * 4, nF=max_id * 12)
        pieces += [(k, t[k], tail_need[k]) for k in CHAIN_TAIL]
        check_layout(pieces, p["bytes"])


# ---- limits: the last accepted value and the first refused one ----

def test_neighbour_limit_and_missing_maps(lib):
    ok = [Img(100, nbs=[1] * 31), Img(100)]
    assert dims(lib, ok, [1, 0])["broken"] == OK and dims(lib, ok, [1, 0])["maxNb"] == 31
    bad = [Img(100, nbs=[1] * 32), Img(100)]
    d = dims(lib, bad, [1, 0])
    assert (d["broken"], d["at"]) == (TOO_MANY_NEIGHBORS, 1)
    assert dims(lib, bad, [1])["broken"] == OK                          # only the images of the order count
    scene = [Img(100), Img(100, maps=False), Img(100, nbs=[0] * 40, maps=False)]
    for order, at in (([0, 1], 1), ([3, 0], 0), ([0, 0, 0xFFFFFFFF], 2), ([0, 2], 1)):   # no maps is reported before too many neighbours
        d = dims(lib, scene, order)
        assert (d["broken"], d["at"]) == (NO_MAPS, at), order


def test_table_limits(lib):
    top = 2 ** 29
    assert dims(lib, [Img(top - 1)], [0])["broken"] == OK
    assert dims(lib, [Img(top)], [0])["broken"] == STRIDE_LIMIT
    d = dims(lib, [Img(100), Img(top)], [0])                           # a map outside the order sets the stride as well
    assert (d["broken"], d["maxArea"], d["stride"]) == (STRIDE_LIMIT, 100, top)
    assert dims(lib, [Img(100), Img(top, maps=False)], [0])["broken"] == OK
    # stride * maxNb against 0x7FFFFFFF.  That number is prime, and a stride it could be a multiple of is beyond 2^29, so the product itself never
    # equals it: the largest product not above it is accepted, the next stride refused
    for nb in (4, 5, 7, 31):
        s = 0x7FFFFFFF // nb
        assert s * nb <= 0x7FFFFFFF < (s + 1) * nb
        d = dims(lib, [Img(100, nbs=[1] * nb), Img(s)], [0])
        assert (d["broken"], d["stride"], d["maxNb"]) == (OK, s, nb)
        d = dims(lib, [Img(100, nbs=[1] * nb), Img(s + 1)], [0])
        assert d["broken"] == (TABLE_LIMIT if s + 1 < top else STRIDE_LIMIT), nb
    assert dims(lib, [Img(100, nbs=[1] * 5), Img(0x7FFFFFFF // 5 + 1)], [0])["broken"] == TABLE_LIMIT


def test_chain_image_and_list_limits(lib):
    top = 2 ** 26 - 1
    for in_order in (False, True):
        order = [0, 1] if in_order else [1]
        assert chain(lib, [Img(top - 1), Img(9), Img(9)], [1, 2], order, scratch=256) is not None
        assert chain(lib, [Img(top), Img(9), Img(9)], [1, 2], order, scratch=256) is None
    # 2 * nNb * n against 0xFFFFFFFF
    nnb = 33
    n0 = -(-0xFFFFFFFF // (2 * nnb))                                  # the first n with 2 * nNb * n >= 0xFFFFFFFF
    assert 2 * nnb * (n0 - 1) < 0xFFFFFFFF <= 2 * nnb * n0 and n0 < top
    assert chain(lib, [Img(n0 - 1, nbs=[9] * nnb), Img(9)], [0, 1], [0], scratch=256) is not None
    assert chain(lib, [Img(n0, nbs=[9] * nnb), Img(9)], [0, 1], [0], scratch=256) is None
    assert chain(lib, [Img(n0, nbs=[9] * nnb), Img(9)], [0, 1], [1], scratch=256) is not None   # only the images of the order have lists
    # nNb * stride against 0xFFFFFFFF (255 x 16843009 is that number itself: all ones means "none", so it is refused)
    for nnb in (65, 255):
        s0 = -(-0xFFFFFFFF // nnb)
        assert nnb * (s0 - 1) < 0xFFFFFFFF <= nnb * s0 and s0 < top
        assert chain(lib, [Img(1, nbs=[1] * nnb), Img(s0 - 1)], [0, 1], [0], scratch=256) is not None
        assert chain(lib, [Img(1, nbs=[1] * nnb), Img(s0)], [0, 1], [0], scratch=256) is None
    assert 255 * s0 == 0xFFFFFFFF
    assert chain(lib, [Img(1, nbs=[1] * nnb), Img(s0, maps=False), Img(9)], [0, 2], [0], scratch=256) is not None   # a neighbour without maps has no list


def test_chain_counts_and_repeats(lib):
    scene = [Img(4)] * 60001
    assert chain(lib, scene, [0], [0, 1]) is None
    assert chain(lib, scene, [0, 1], [0, 1]) is not None
    assert chain(lib, scene, list(range(2000)), [0, 1]) is not None
    assert chain(lib, scene, list(range(2001)), [0, 1]) is None
    assert chain(lib, scene, [0, 1], list(range(60000))) is not None
    assert chain(lib, scene, [0, 1], list(range(60001))) is None
    assert chain(lib, scene, [5, 6, 5], [0, 1]) is None               # a repeated id
    assert chain(lib, scene, [5, 6, 7], [0, 1, 0]) is None            # a repeated order entry
    assert chain(lib, scene, [5, 6, 7], [7, 1, 0]) is not None
