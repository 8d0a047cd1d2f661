"""diagnostic (not a test): time hcmvs_select_views on the sparse cloud of the BASELINE.json configs[2] scene (64 images of 1920 x 1080 on
two rings, built as tests/test_gpu_configs.py::ring_scene builds it: 400 points sampled on every 4th view) and on a denser cloud of the
same cameras, beside the driver's host loop (host/driver_plan.h select_views for every image, through tests/driver_plan_shim.cpp built
with -O2: ONE thread -- the driver spreads the images over its OpenMP threads).  One JSON line per cloud.
usage: view_select_bench.py [images] [dense points per view]"""
import ctypes as C
import importlib, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import scene_files as SF
binding = importlib.import_module("hc-mvs_amd.binding")
synth = importlib.import_module("hc-mvs_amd.synth")

N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
DENSE = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
W, H = 1920, 1080
t0 = time.perf_counter()
f = 1600.0 * W / 1920
px = 10.0 / f
scene = synth.Scene(3, min_wavelength=3.5 * px, max_wavelength=150 * px)
K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1]], np.float64)
target = np.array([0.0, 0.0, scene.depth0])
rng = np.random.RandomState(11)
poses = []
for i in range(N):
    ang = 2 * np.pi * (i // 2) / (N // 2)
    rad = scene.depth0 * (0.10 + 0.06 * (i % 2))
    Cc = np.array([rad * np.cos(ang), rad * np.sin(ang) * 0.7, 0.01 * rng.uniform(-1, 1)])
    poses.append((synth.look_at(Cc, target), Cc))
views = SF.render_views(scene, K, poses, W, H, threads=12)
t1 = time.perf_counter()

tmp = tempfile.mkdtemp()
shim = os.path.join(tmp, "libdriver_plan_shim.so")
subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-shared", "-fPIC", "-o", shim, os.path.join(ROOT, "tests", "driver_plan_shim.cpp")])
L = C.CDLL(shim)
PD, PF, PI, PU = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_uint32)
L.dp_select_views.argtypes = [C.c_int, C.c_int, C.c_int, PD, PD, PD, C.c_int, C.c_int, C.c_int, PF, PI, PU, C.c_int, C.c_int]
L.dp_select_views.restype = C.c_char_p

cams = [dict(K=v["K"], R=v["R"], C=v["C"]) for v in views]
sizes = [(W, H)] * N
Rs = np.ascontiguousarray(np.stack([v["R"] for v in views]).reshape(N, 9)); Cs = np.ascontiguousarray(np.stack([v["C"] for v in views]))
Kn = np.ascontiguousarray(K.ravel())
ctx = binding.Context(0)
for label, per_view, every in (("configs[2]", 400, 4), ("dense", DENSE, 1)):
    verts = SF.sparse_vertices(views, per_view, every=every, seed=11)
    xyz = np.ascontiguousarray(np.stack([v["X"] for v in verts]), np.float32)
    nv = np.array([len(v["views"]) for v in verts], np.uint32)
    ids = np.array([j for v in verts for j, _ in v["views"]], np.uint32)
    first = np.concatenate([[0], np.cumsum(nv, dtype=np.int64)]).astype(np.int32)
    for rep in range(2):  # the first call pays the kernels' first load
        t2 = time.perf_counter()
        r = ctx.select_views_raw(cams, sizes, xyz, nv, ids, number_views=8)
        t3 = time.perf_counter()
    t4 = time.perf_counter()
    # the shim's one camera is K at W x H with R = I, C = 0; the poses carry the cameras
    text = L.dp_select_views(N, W, H, Kn.ctypes.data_as(PD), Rs.ctypes.data_as(PD), Cs.ctypes.data_as(PD), W, H, len(verts), xyz.ctypes.data_as(PF),
                             first.ctypes.data_as(PI), ids.ctypes.data_as(PU), 12, 8).decode()
    t5 = time.perf_counter()
    host_srcs = [[int(x) for x in ln.split("|")[1].split()] for ln in text.strip().splitlines()]
    dev_srcs = [[int(x) for x in r["nb_id"][i, :r["n_srcs"][i]]] for i in range(N)]
    st = r["stats"]
    print(json.dumps(dict(cloud=label, images=N, points=len(verts), view_entries=len(ids), pairs=st["pairs"], chunks=st["chunks"],
                          ms_device=round(st["ms_device"], 3), device_mib=round(st["device_bytes"] / 2 ** 20, 2), call_wall_ms=round((t3 - t2) * 1e3, 2),
                          host_loop_one_thread_ms=round((t5 - t4) * 1e3, 2), same_source_views=host_srcs == dev_srcs, selected=int((r["status"] == 0).sum()),
                          render_s=round(t1 - t0, 1))), flush=True)
ctx.close()
