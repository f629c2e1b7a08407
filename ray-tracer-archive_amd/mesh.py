"""Triangle meshes with per-vertex normals and texture coordinates: a procedural sphere mesh, and the numpy restatement of what the
library does with RtTriangleAttrs (include/rt_hip.h "triangle attributes") — usable at f64 as the definition and at f32 as the
arithmetic the device performs. Nothing here touches the device."""
import numpy as np

from . import _abi as A


def icosphere(subdivisions):
    """(tris (n, 3, 3) f64, normals (n, 3, 3) f64) of the unit sphere about the origin: an icosahedron whose faces are split in four
    `subdivisions` times, every new vertex pushed out to the sphere. 20 * 4**subdivisions triangles, wound counter-clockwise seen from
    outside; the vertex normals are the vertices themselves."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [np.array(v, dtype=np.float64) for v in
             [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]]
    verts = [v / np.linalg.norm(v) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(int(subdivisions)):
        middle = {}

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in middle:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                middle[key] = len(verts) - 1
            return middle[key]
        split = []
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            split += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = split
    tris = np.array(verts)[np.array(faces)]
    return tris, tris.copy()


def sphere_uv(n):
    """(u, v) of the unit vectors n (..., 3) as Sphere::get_sphere_uv gives them (sphere.rs:32-37), for texturing a sphere mesh. Returns (..., 2)."""
    n = np.asarray(n, dtype=np.float64)
    theta = np.arccos(np.clip(-n[..., 1], -1.0, 1.0))
    phi = np.arctan2(-n[..., 2], n[..., 0]) + np.pi
    return np.stack([phi / (2.0 * np.pi), theta / np.pi], axis=-1)


def _outward(tris, attrs, hittable, bu, bv, T):
    """(outward (N, 3), u (N,), v (N,)) of interpolate_reference before the face test: the unit normal and the texture coordinates the
    RT_TRI_NORMALS and RT_TRI_UVS steps leave, in the operations and order of csrc/kernels.hip tri_attr_apply."""
    by_id = {int(a.hittable): a for a in (attrs if attrs is not None else ())}
    N = len(hittable)
    out, u, v = np.zeros((N, 3), T), bu.copy(), bv.copy()
    tiny = T(np.finfo(np.float32).tiny)          # the device's test is made in f32

    def unit(x):
        return x / np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]).astype(T))[:, None]
    for h in np.unique(hittable):
        k = np.flatnonzero(hittable == h)
        P = np.asarray(tris[int(h)], dtype=np.float64).astype(T).reshape(3, 3)
        o = np.broadcast_to(unit(np.cross(P[1] - P[0], P[2] - P[0]).astype(T)[None, :]), (len(k), 3)).copy()
        a = by_id.get(int(h))
        if a is not None and a.flags & A.RT_TRI_NORMALS:
            vn = np.array([[a.n[i][c] for c in range(3)] for i in range(3)], dtype=np.float64)
            vn = (vn / np.linalg.norm(vn, axis=1, keepdims=True)).astype(T)
            w0 = (T(1.0) - bu[k] - bv[k]).astype(T)
            s = ((w0[:, None] * vn[0] + bu[k][:, None] * vn[1]).astype(T) + bv[k][:, None] * vn[2]).astype(T)
            l2 = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2]).astype(T)
            ok = (l2 >= tiny) & np.isfinite(l2)
            o[ok] = unit(s[ok])
        if a is not None and a.flags & A.RT_TRI_UVS:
            uv = np.array([[a.uv[i][c] for c in range(2)] for i in range(3)], dtype=np.float32).astype(T)
            u[k] = ((uv[0, 0] + bu[k] * (uv[1, 0] - uv[0, 0])).astype(T) + bv[k] * (uv[2, 0] - uv[0, 0])).astype(T)
            v[k] = ((uv[0, 1] + bu[k] * (uv[1, 1] - uv[0, 1])).astype(T) + bv[k] * (uv[2, 1] - uv[0, 1])).astype(T)
        out[k] = o
    return out, u, v


def _face(out, d, T):
    front = (d[:, 0] * out[:, 0] + d[:, 1] * out[:, 1] + d[:, 2] * out[:, 2]).astype(T) < 0
    return np.where(front[:, None], out, -out), front


def interpolate_reference(tris, attrs, hittable, bu, bv, d, dtype=np.float64):
    """The HitRecord fields RtTriangleAttrs decide, for N hits, in the triangle's own (pre-wrapper) space, every operation in `dtype`:

        tris      {hittable id: (3, 3) vertices} (or anything indexable by id)
        attrs     RtTriangleAttrs records (a triangle without one, or with flags 0, is a plain triangle)
        hittable  (N,) ids of the triangles hit;  bu, bv (N,) the barycentrics tri_hit returns;  d (N, 3) the ray's direction

    Returns (n (N, 3), front_face (N,), u (N,), v (N,)): ns = unit(w0 n0 + bu n1 + bv n2) with w0 = 1 - bu - bv and the vertex normals made
    unit in f64 and then rounded to `dtype` — or the geometric normal where the flag is clear or the squared length of the sum is not a
    positive normal number; front_face = dot(d, ns) < 0; n = +-ns, against the ray; u = u0 + bu (u1 - u0) + bv (u2 - u0), v likewise, or
    (bu, bv) without RT_TRI_UVS. The operations and their order are those of csrc/kernels.hip tri_attr_apply."""
    T = np.dtype(dtype).type
    hittable = np.asarray(hittable).astype(np.int64)
    bu, bv, d = np.asarray(bu).astype(T), np.asarray(bv).astype(T), np.asarray(d).astype(T).reshape(-1, 3)
    out, u, v = _outward(tris, attrs, hittable, bu, bv, T)
    n, ff = _face(out, d, T)
    return n, ff, u, v


def texel_of(u, v, width, height, dtype=np.float64):
    """(i, j) of the image texture's rule (texture.rs:117-140) in `dtype`: u, v clamped to [0, 1], v := 1 - v, i = (uint)(u W), j = (uint)(v H),
    clamped to W - 1, H - 1. Row 0 of the image is v = 1."""
    T = np.dtype(dtype).type
    u = np.minimum(np.maximum(np.asarray(u).astype(T), T(0.0)), T(1.0))
    v = (T(1.0) - np.minimum(np.maximum(np.asarray(v).astype(T), T(0.0)), T(1.0))).astype(T)
    i = np.minimum((u * T(width)).astype(T).astype(np.int64), width - 1)
    j = np.minimum((v * T(height)).astype(T).astype(np.int64), height - 1)
    return i, j


def normal_map_reference(tris, attrs, hittable, bu, bv, image, strength=1.0, flip_green=False, dtype=np.float64, d=None, frame=False):
    """What a normal map (include/rt_hip.h RtNormalMap, steps TEXEL, DECODE, FRAME, RESULT, FALLBACKS) makes of N hits on triangles whose
    material carries it, on top of interpolate_reference and with its arguments; image: the map's (H, W, 3) uint8 texels. Every operation
    in `dtype`, in the order of csrc/kernels.hip normal_map_apply.

    Returns (n (N, 3), front_face (N,), u (N,), v (N,), texel (N,)): texel = j W + i, the texel read (so that a test can tell the hits
    on a texel boundary apart); with d (N, 3), the ray's direction in the triangle's space, n = +-ns against the ray and front_face =
    dot(d, ns) < 0; without it n = ns, the mapped outward normal, and front_face is None. frame=True appends (t, b, N, ok), each (N, ...):
    the tangent frame of step FRAME and whether the map was applied (False: a fallback left N; t, b are then 0 or meaningless)."""
    T = np.dtype(dtype).type
    hittable = np.asarray(hittable).astype(np.int64)
    bu, bv = np.asarray(bu).astype(T), np.asarray(bv).astype(T)
    image = np.asarray(image, dtype=np.uint8)
    H, W, _ = image.shape
    out, u, v = _outward(tris, attrs, hittable, bu, bv, T)
    i, j = texel_of(u, v, W, H, T)
    c = image[j, i].astype(T)
    k255 = T(T(2.0) / T(255.0))
    m = (c * k255).astype(T) - T(1.0)
    x, y, z = (T(strength) * m[:, 0]).astype(T), (T(strength) * m[:, 1]).astype(T), m[:, 2].astype(T)
    if flip_green:
        y = -y
    tiny = T(np.finfo(np.float32).tiny)
    by_id = {int(a.hittable): a for a in (attrs if attrs is not None else ())}
    fr_t, fr_b, fr_n, fr_ok = np.zeros_like(out), np.zeros_like(out), out.copy(), np.zeros(len(out), bool)

    def dot(a, b):
        return ((a[:, 0] * b[:, 0]).astype(T) + (a[:, 1] * b[:, 1]).astype(T) + (a[:, 2] * b[:, 2]).astype(T)).astype(T)

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], -(a[:, 0] * b[:, 2] - a[:, 2] * b[:, 0]), a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(T)
    for h in np.unique(hittable):
        k = np.flatnonzero(hittable == h)
        P = np.asarray(tris[int(h)], dtype=np.float64).astype(T).reshape(3, 3)
        a = by_id.get(int(h))
        if a is not None and a.flags & A.RT_TRI_UVS:
            uv = np.array([[a.uv[q][c] for c in range(2)] for q in range(3)], dtype=np.float32).astype(T)
        else:
            uv = np.array([[0, 0], [1, 0], [0, 1]], dtype=T)
        du1, dv1, du2, dv2 = T(uv[1, 0] - uv[0, 0]), T(uv[1, 1] - uv[0, 1]), T(uv[2, 0] - uv[0, 0]), T(uv[2, 1] - uv[0, 1])
        det = T(T(du1 * dv2) - T(du2 * dv1))
        if not (det != 0 and np.isfinite(det)):
            continue                                                            # collinear uv: N stays
        e1, e2 = (P[1] - P[0]).astype(T), (P[2] - P[0]).astype(T)
        Tv, Bv = ((dv2 * e1).astype(T) - (dv1 * e2).astype(T)).astype(T), ((du1 * e2).astype(T) - (du2 * e1).astype(T)).astype(T)
        if det < 0:
            Tv, Bv = -Tv, -Bv
        N = out[k]
        Tn, Bn = np.broadcast_to(Tv, N.shape), np.broadcast_to(Bv, N.shape)
        tp = (Tn - (N * dot(N, Tn)[:, None]).astype(T)).astype(T)
        tl2 = dot(tp, tp)
        ok = (tl2 >= tiny) & np.isfinite(tl2)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = (tp / np.sqrt(tl2)[:, None]).astype(T)
        b = cross(N, t)
        b = np.where((dot(b, Bn) < 0)[:, None], -b, b)
        s = (((x[k][:, None] * t).astype(T) + (y[k][:, None] * b).astype(T)).astype(T) + (z[k][:, None] * N).astype(T)).astype(T)
        sl2 = dot(s, s)
        ok &= (sl2 >= tiny) & np.isfinite(sl2)
        with np.errstate(invalid="ignore", divide="ignore"):
            ns = (s / np.sqrt(sl2)[:, None]).astype(T)
        out[k] = np.where(ok[:, None], ns, N)
        fr_t[k], fr_b[k], fr_ok[k] = t, b, ok
    texel = j * W + i
    more = ((fr_t, fr_b, fr_n, fr_ok),) if frame else ()
    if d is None:
        return (out, None, u, v, texel) + more
    n, ff = _face(out, np.asarray(d).astype(T).reshape(-1, 3), T)
    return (n, ff, u, v, texel) + more


def height_to_normal_map(height, scale=1.0):
    """An (H, W, 3) uint8 normal map of a 2-D height array (row 0 = the top of the image, v = 1), by central differences (one-sided at the
    borders): n = unit(-scale dh/du, -scale dh/dv, 1) with du, dv one texel, +v towards row 0, encoded as the library decodes it
    (c = round((n + 1) 255 / 2): red = +u, green = +v, blue = along the normal)."""
    h = np.asarray(height, dtype=np.float64)
    dhdx = np.gradient(h, axis=1) if h.shape[1] > 1 else np.zeros_like(h)
    dhdy = -np.gradient(h, axis=0) if h.shape[0] > 1 else np.zeros_like(h)       # rows run down, v runs up
    n = np.stack([-scale * dhdx, -scale * dhdy, np.ones_like(h)], axis=-1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    return np.clip(np.rint((n + 1.0) * 127.5), 0, 255).astype(np.uint8)
