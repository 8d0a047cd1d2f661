"""numpy restatement of Mesh::SamplePoints (frame_main/libs/MVS/Mesh.cpp:3444-3527; DensifyPointCloud --sample-mesh), the spec
hcmvs_sample_mesh is checked against bit for bit: the counter-based draws of DESIGN.md section 5 (D11) in place of the reference's
unseeded std::mt19937, and the reference's arithmetic with the association DESIGN.md states.  Test infrastructure, no GPU."""
import numpy as np

F = np.float32
U64 = np.uint64
ZEROTOLERANCE_F = float(F(0.0001))  # ZEROTOLERANCE<float>() (Types.h:572, 1196)


def mix(z):
    """the splitmix64 step on uint64, wrap-around"""
    z = np.asarray(z, U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def draw(seed, face, k):
    """draw k of face `face` under `seed`: a double in [0, 1)"""
    with np.errstate(over="ignore"):
        a = mix(U64(seed) ^ mix(face))
        z = mix(a + np.asarray(k, U64) * U64(0xD1B54A32D192ED03))
    return (z >> U64(11)).astype(np.float64) * 2.0 ** -53


def edges(vertices, faces):
    V = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    Fc = np.asarray(faces, np.int64).reshape(-1, 3)
    O = V[Fc[:, 0]]
    return O, V[Fc[:, 1]] - O, V[Fc[:, 2]] - O


def cross(u, v):
    """cv::Point3f::cross: every component a*b - c*d in float32, products rounded"""
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], -1)


def face_areas(vertices, faces):
    """(float32 ComputeTriangleArea per face (Util.inl:476-482), float64 norm(u x v) * 0.5 per face (Mesh.cpp:3488))"""
    with np.errstate(over="ignore", invalid="ignore"):
        _, u, v = edges(vertices, faces)
        c = cross(u, v)
        area_f = np.sqrt(((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]) / F(4))
        d = c.astype(np.float64)
        area_d = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) * 0.5  # cv::norm(Point3f) accumulates in double
    assert area_f.dtype == F
    return area_f, area_d


def total_area(area_f):
    """Mesh::ComputeArea (Mesh.cpp:3423-3429): the float areas added to a double one after the other, in face order"""
    s = 0.0
    for a in area_f.astype(np.float64).tolist():
        s += a
    return s


def density_of(vertices, faces, sample):
    """(density, total area); density None: Mesh::SamplePoints(unsigned) returns an empty cloud (area < ZEROTOLERANCE<float>())"""
    area = total_area(face_areas(vertices, faces)[0])
    s = float(F(sample))
    if s > 0:
        return s, area
    n = int(np.floor(F(-s) + F(0.5)))  # ROUND2INT(-sample) = Round2Int(float): int(floor(x + .5f)), in float (Types.h:937-943)
    if area < ZEROTOLERANCE_F:
        return None, area
    return n / area, area


def counts(vertices, faces, density, seed):
    """points per face: (unsigned)(area * density), one more when draw 0 <= the fractional part"""
    _, area_d = face_areas(vertices, faces)
    with np.errstate(invalid="ignore", over="ignore"):
        fp = area_d * density
        ok = fp < 4294967296.0  # NaN: no point; the device refuses a cloud of 2^32 points or more
        n = np.where(ok, fp, 0.0).astype(U64)
        n = np.where(ok | np.isnan(fp), n, U64(1 << 32))
        frac = fp - n.astype(np.float64)
        n = n + (draw(seed, np.arange(len(n), dtype=U64), 0) <= frac).astype(U64)
    return n, fp


def sat_int(v):
    """float32 -> int32, truncating, saturating, NaN -> 0 (defined where the reference's (int) cast is not)"""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore"):
        out = np.where(np.isnan(v), F(0), np.clip(v, F(-2147483648.0), F(2147483520.0))).astype(np.int64)
    return np.where(v >= F(2147483648.0), 2147483647, out)


def u8(v):
    """(uint8_t)(float): truncation; outside [0, 256) the low byte of the saturated int"""
    return (sat_int(v) & 255).astype(np.uint8)


def sample_texture(tex, px, py):
    """TImage<Pixel8U>::sampleSafe (Types.inl:2261-2269) over getPixel (:2232-2243), every step of the Pixel8U arithmetic truncated back to
    8 bits (Types.h:1930-1937) the way hcmvs_estimate_point_colors restates its sample"""
    h, w, _ = tex.shape
    lx, ly = sat_int(px), sat_int(py)
    x = px - lx.astype(F); x1 = F(1) - x
    y = py - ly.astype(F); y1 = F(1) - y
    def pix(yy, xx):
        return tex[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(F)
    x, x1, y, y1 = x[:, None], x1[:, None], y[:, None], y1[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        top = u8((u8(x1 * pix(ly, lx)) + u8(x * pix(ly, lx + 1))).astype(F) * y1)
        bot = u8((u8(x1 * pix(ly + 1, lx)) + u8(x * pix(ly + 1, lx + 1))).astype(F) * y)
    return top + bot  # uint8, wraps


def sample_mesh(vertices, faces, sample, seed=0, texcoords=None, texture_bgr=None):
    """-> dict(xyz (n, 3) f32, face (n,) u32, bgr (n, 3) u8 or None, counts per face, x, y (the folded barycentrics, f64), area, density)"""
    V = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    Fc = np.asarray(faces, np.int64).reshape(-1, 3)
    density, area = density_of(V, Fc, sample)
    if density is None:
        return dict(xyz=np.zeros((0, 3), F), face=np.zeros(0, np.uint32), bgr=None if texture_bgr is None else np.zeros((0, 3), np.uint8),
                    counts=np.zeros(len(Fc), U64), x=np.zeros(0), y=np.zeros(0), area=area, density=0.0)
    n, _ = counts(V, Fc, density, seed)
    total = int(n.sum())
    assert total < 1 << 32
    face = np.repeat(np.arange(len(Fc), dtype=np.int64), n.astype(np.int64))
    first = np.concatenate([[0], np.cumsum(n.astype(np.int64))])[:-1]
    i = np.arange(total, dtype=np.int64) - first[face]
    x = draw(seed, face.astype(U64), (1 + 2 * i).astype(U64))
    y = draw(seed, face.astype(U64), (2 + 2 * i).astype(U64))
    fold = x + y > 1.0
    x = np.where(fold, 1.0 - x, x); y = np.where(fold, 1.0 - y, y)
    fx, fy = x.astype(F)[:, None], y.astype(F)[:, None]
    O, u, v = edges(V, Fc)
    with np.errstate(over="ignore", invalid="ignore"):
        xyz = (O[face] + fx * u[face]) + fy * v[face]
    assert xyz.dtype == F
    bgr = None
    if texture_bgr is not None:
        tex = np.ascontiguousarray(texture_bgr, np.uint8)
        T = np.ascontiguousarray(texcoords, F).reshape(-1, 3, 2)[face]
        with np.errstate(over="ignore", invalid="ignore"):
            xt = (T[:, 0] + fx * (T[:, 1] - T[:, 0])) + fy * (T[:, 2] - T[:, 0])
            bgr = sample_texture(tex, xt[:, 0] * F(tex.shape[1]), (F(1) - xt[:, 1]) * F(tex.shape[0]))
    return dict(xyz=xyz, face=face.astype(np.uint32), bgr=bgr, counts=n, x=x, y=y, area=area, density=density)
