"""File formats at the boundary of the densify path: the `.mvs` scene (MVSI v5,
Interface.h:212-231, 363-619), the raw 'DR' depth map (Interface.h:634-652, writer DepthMap.cpp:2781-2846) and the
binary little-endian PLY point cloud (PointCloud.cpp:105-240).  Pure struct/numpy code, no third-party readers."""
import struct

import numpy as np

MVSI_VERSION = 5


def _w_str(f, s):
    b = s.encode()
    f.write(struct.pack("<Q", len(b))); f.write(b)


def _r_str(f):
    n, = struct.unpack("<Q", f.read(8))
    return f.read(n).decode()


def write_mvs(path, platforms, images, vertices=(), colors=(), normals=()):
    """platforms: [dict(name, cameras=[dict(name, width, height, K(3,3), R(3,3), C(3))], poses=[dict(R, C)])]
    images: [dict(name, platformID, cameraID, poseID, ID, maskName='')]
    vertices: [dict(X(3), views=[(imageID, confidence)])]; colors: (n,3) u8 B,G,R; normals: (n,3) f32"""
    with open(path, "wb") as f:
        f.write(b"MVSI"); f.write(struct.pack("<II", MVSI_VERSION, 0))
        f.write(struct.pack("<Q", len(platforms)))
        for p in platforms:
            _w_str(f, p["name"])
            f.write(struct.pack("<Q", len(p["cameras"])))
            for c in p["cameras"]:
                _w_str(f, c["name"]); _w_str(f, c.get("bandName", ""))
                f.write(struct.pack("<II", c["width"], c["height"]))
                f.write(np.asarray(c["K"], "<f8").tobytes()); f.write(np.asarray(c["R"], "<f8").tobytes())
                f.write(np.asarray(c["C"], "<f8").tobytes())
            f.write(struct.pack("<Q", len(p["poses"])))
            for q in p["poses"]:
                f.write(np.asarray(q["R"], "<f8").tobytes()); f.write(np.asarray(q["C"], "<f8").tobytes())
        f.write(struct.pack("<Q", len(images)))
        for im in images:
            _w_str(f, im["name"]); _w_str(f, im.get("maskName", ""))
            f.write(struct.pack("<IIII", im["platformID"], im["cameraID"], im["poseID"], im["ID"]))
        f.write(struct.pack("<Q", len(vertices)))
        for v in vertices:
            f.write(np.asarray(v["X"], "<f4").tobytes())
            f.write(struct.pack("<Q", len(v["views"])))
            for iid, conf in v["views"]:
                f.write(struct.pack("<If", iid, conf))
        normals = np.asarray(normals, "<f4").reshape(-1, 3)
        f.write(struct.pack("<Q", len(normals))); f.write(normals.tobytes())
        colors = np.asarray(colors, np.uint8).reshape(-1, 3)
        f.write(struct.pack("<Q", len(colors))); f.write(colors.tobytes())
        for _ in range(3):  # lines, linesNormal, linesColor
            f.write(struct.pack("<Q", 0))
        f.write(np.eye(4, dtype="<f8").tobytes())  # transform (version > 1)


def read_mvs(path):
    with open(path, "rb") as f:
        assert f.read(4) == b"MVSI"
        ver, _ = struct.unpack("<II", f.read(8))
        assert ver == MVSI_VERSION, "only MVSI v5 is handled"
        out = dict(version=ver, platforms=[], images=[], vertices=[])
        for _ in range(struct.unpack("<Q", f.read(8))[0]):
            p = dict(name=_r_str(f), cameras=[], poses=[])
            for _ in range(struct.unpack("<Q", f.read(8))[0]):
                c = dict(name=_r_str(f), bandName=_r_str(f))
                c["width"], c["height"] = struct.unpack("<II", f.read(8))
                c["K"] = np.frombuffer(f.read(72), "<f8").reshape(3, 3).copy()
                c["R"] = np.frombuffer(f.read(72), "<f8").reshape(3, 3).copy()
                c["C"] = np.frombuffer(f.read(24), "<f8").copy()
                p["cameras"].append(c)
            for _ in range(struct.unpack("<Q", f.read(8))[0]):
                p["poses"].append(dict(R=np.frombuffer(f.read(72), "<f8").reshape(3, 3).copy(), C=np.frombuffer(f.read(24), "<f8").copy()))
            out["platforms"].append(p)
        for _ in range(struct.unpack("<Q", f.read(8))[0]):
            im = dict(name=_r_str(f), maskName=_r_str(f))
            im["platformID"], im["cameraID"], im["poseID"], im["ID"] = struct.unpack("<IIII", f.read(16))
            out["images"].append(im)
        for _ in range(struct.unpack("<Q", f.read(8))[0]):
            X = np.frombuffer(f.read(12), "<f4").copy()
            views = [struct.unpack("<If", f.read(8)) for _ in range(struct.unpack("<Q", f.read(8))[0])]
            out["vertices"].append(dict(X=X, views=views))
        n, = struct.unpack("<Q", f.read(8)); out["normals"] = np.frombuffer(f.read(12 * n), "<f4").reshape(-1, 3).copy()
        n, = struct.unpack("<Q", f.read(8)); out["colors"] = np.frombuffer(f.read(3 * n), np.uint8).reshape(-1, 3).copy()
        return out


def image_camera(scene, idx):
    """composed K, R, C of image idx (Interface.h:451-459, Platform.cpp:43-53): R = Rcam Rpose, C = Rpose^T Ccam + Cpose"""
    im = scene["images"][idx]
    p = scene["platforms"][im["platformID"]]
    cam, pose = p["cameras"][im["cameraID"]], p["poses"][im["poseID"]]
    return cam["K"], cam["R"] @ pose["R"], pose["R"].T @ cam["C"] + pose["C"], cam["width"], cam["height"]


def write_dmap(path, depth, K, R, C, d_min, d_max, ids, image_name="", normal=None, conf=None, image_size=None):
    """raw 'DR' depth map (Interface.h:634-652): 28-byte header, name, ids (reference first), K, R, C, maps"""
    h, w = depth.shape
    iw, ih = image_size if image_size else (w, h)
    typ = 1 | (2 if normal is not None else 0) | (4 if conf is not None else 0)
    with open(path, "wb") as f:
        f.write(struct.pack("<HBBIIIIff", 0x5244, typ, 0, iw, ih, w, h, d_min, d_max))
        b = image_name.encode(); f.write(struct.pack("<H", len(b))); f.write(b)
        f.write(struct.pack("<I", len(ids))); f.write(np.asarray(ids, "<u4").tobytes())
        f.write(np.asarray(K, "<f8").tobytes()); f.write(np.asarray(R, "<f8").tobytes()); f.write(np.asarray(C, "<f8").tobytes())
        f.write(np.ascontiguousarray(depth, "<f4").tobytes())
        if normal is not None:
            f.write(np.ascontiguousarray(normal, "<f4").tobytes())
        if conf is not None:
            f.write(np.ascontiguousarray(conf, "<f4").tobytes())


def read_dmap(path):
    with open(path, "rb") as f:
        name, typ, _, iw, ih, w, h, dmin, dmax = struct.unpack("<HBBIIIIff", f.read(28))
        assert name == 0x5244, "not a raw 'DR' depth map"
        n, = struct.unpack("<H", f.read(2)); img = f.read(n).decode()
        n, = struct.unpack("<I", f.read(4)); ids = np.frombuffer(f.read(4 * n), "<u4").copy()
        K = np.frombuffer(f.read(72), "<f8").reshape(3, 3).copy(); R = np.frombuffer(f.read(72), "<f8").reshape(3, 3).copy()
        C = np.frombuffer(f.read(24), "<f8").copy()
        out = dict(image_name=img, ids=ids, K=K, R=R, C=C, d_min=dmin, d_max=dmax, image_size=(iw, ih))
        out["depth"] = np.frombuffer(f.read(4 * w * h), "<f4").reshape(h, w).copy()
        if typ & 2:
            out["normal"] = np.frombuffer(f.read(12 * w * h), "<f4").reshape(h, w, 3).copy()
        if typ & 4:
            out["conf"] = np.frombuffer(f.read(4 * w * h), "<f4").reshape(h, w).copy()
        return out


def write_ply(path, xyz, bgr=None, normal=None):
    """binary little-endian PLY: x y z f32 [nx ny nz f32] [red green blue u8] (PointCloud.cpp:189-240)"""
    n = len(xyz)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normal is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if bgr is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.zeros(n, np.dtype(fields))
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normal is not None:
        rec["nx"], rec["ny"], rec["nz"] = normal[:, 0], normal[:, 1], normal[:, 2]
    if bgr is not None:
        rec["red"], rec["green"], rec["blue"] = bgr[:, 2], bgr[:, 1], bgr[:, 0]
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n)
        for nm, t in fields:
            f.write(("property %s %s\n" % ("float" if t == "<f4" else "uchar", nm)).encode())
        f.write(b"end_header\n")
        f.write(rec.tobytes())


def read_ply(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"ply"
        props, n = [], 0
        while True:
            ln = f.readline().strip().decode()
            if ln.startswith("element vertex"):
                n = int(ln.split()[-1])
            elif ln.startswith("property"):
                _, t, nm = ln.split()
                props.append((nm, "<f4" if t in ("float", "float32") else "u1"))
            elif ln == "end_header":
                break
        return np.frombuffer(f.read(), np.dtype(props), count=n)


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2", "int": "<i4",
              "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8"}


def write_ply_mesh(path, vertices, faces, texcoords=None, texture_file=None, ascii=False, index_type="int", list_name="vertex_indices"):
    """PLY triangle mesh as Mesh::SavePLY writes it (Mesh.cpp:1513-1600): vertex x y z f32, face list uchar <index_type> <list_name>,
    optionally list uchar float texcoord (6 per face: u v of the three corners) and "comment TextureFile <texture_file>"; binary
    little-endian or ascii (floats with 9 significant digits: they read back exactly)"""
    V = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    Fc = np.ascontiguousarray(faces).reshape(-1, 3)
    T = None if texcoords is None else np.ascontiguousarray(texcoords, np.float32).reshape(-1, 6)
    assert T is None or len(T) == len(Fc)
    it = _PLY_TYPES[index_type]
    head = "ply\nformat %s 1.0\n" % ("ascii" if ascii else "binary_little_endian")
    if texture_file:
        head += "comment TextureFile %s\n" % texture_file
    head += "element vertex %d\nproperty float x\nproperty float y\nproperty float z\nelement face %d\nproperty list uchar %s %s\n" % (len(V), len(Fc), index_type, list_name)
    if T is not None:
        head += "property list uchar float texcoord\n"
    head += "end_header\n"
    with open(path, "wb") as f:
        f.write(head.encode())
        if ascii:
            for v in V:
                f.write(("%.9g %.9g %.9g\n" % tuple(v.tolist())).encode())
            for k, fc in enumerate(Fc):
                ln = "3 %d %d %d" % tuple(int(i) for i in fc)
                if T is not None:
                    ln += " 6 " + " ".join("%.9g" % t for t in T[k].tolist())
                f.write((ln + "\n").encode())
        else:
            f.write(V.astype("<f4").tobytes())
            fields = [("n", "u1"), ("i", it, 3)] + ([("m", "u1"), ("t", "<f4", 6)] if T is not None else [])
            rec = np.zeros(len(Fc), np.dtype(fields))
            rec["n"] = 3; rec["i"] = Fc
            if T is not None:
                rec["m"] = 6; rec["t"] = T
            f.write(rec.tobytes())


def read_ply_mesh(path):
    """-> dict(vertices (n, 3) f32, faces (m, 3) u32, texcoords (m, 3, 2) f32 or None, texture_file or None); ascii or binary little-endian,
    vertex properties beyond x y z are skipped; a face that is not a triangle is an error"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header")
    end = data.index(b"\n", end) + 1
    lines = [ln.strip() for ln in data[:end].decode("latin-1").split("\n")]
    if lines[0] != "ply":
        raise ValueError("not a PLY file")
    fmt, tex_file, elements = None, None, []
    for ln in lines[1:]:
        w = ln.split()
        if not w:
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "comment" and len(w) >= 3 and w[1] == "TextureFile":
            tex_file = ln.split("TextureFile", 1)[1].strip()
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property":
            elements[-1][2].append((w[4], _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]) if w[1] == "list" else (w[2], None, _PLY_TYPES[w[1]]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError("unsupported PLY format %r" % fmt)
    out = dict(vertices=None, faces=None, texcoords=None, texture_file=tex_file)
    pos = end
    tokens = iter(data[end:].split()) if fmt == "ascii" else None

    def take(t, n=1):
        nonlocal pos
        if tokens is not None:
            return [float(next(tokens)) for _ in range(n)]
        a = np.frombuffer(data, t, n, pos)
        pos += a.nbytes
        return a.tolist()

    for name, count, props in elements:
        if name == "vertex" and fmt != "ascii" and all(c is None for _, c, _ in props):
            rec = np.frombuffer(data, np.dtype([(nm, t) for nm, _, t in props]), count, pos)
            pos += rec.nbytes
            out["vertices"] = np.stack([rec["x"], rec["y"], rec["z"]], -1).astype(np.float32)
            continue
        rows = {nm: [] for nm, _, _ in props}
        for _ in range(count):
            for nm, ct, t in props:
                rows[nm].append(take(t)[0] if ct is None else take(t, int(take(ct)[0])))
        if name == "vertex":
            out["vertices"] = np.stack([np.asarray(rows[k], np.float64) for k in "xyz"], -1).astype(np.float32).reshape(-1, 3)
        elif name == "face":
            key = "vertex_indices" if "vertex_indices" in rows else "vertex_index"
            if any(len(r) != 3 for r in rows[key]):
                raise ValueError("a face that is not a triangle")
            out["faces"] = np.asarray(rows[key], np.float64).astype(np.uint32).reshape(-1, 3)
            if "texcoord" in rows:
                out["texcoords"] = np.asarray(rows["texcoord"], np.float64).astype(np.float32).reshape(-1, 3, 2)
    if out["vertices"] is None or out["faces"] is None:
        raise ValueError("the PLY file has no vertex or no face element")
    return out


def write_pgm(path, gray_u8):
    h, w = gray_u8.shape
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (w, h)); f.write(np.ascontiguousarray(gray_u8, np.uint8).tobytes())


def write_ppm(path, rgb_u8):
    h, w, _ = rgb_u8.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h)); f.write(np.ascontiguousarray(rgb_u8, np.uint8).tobytes())
