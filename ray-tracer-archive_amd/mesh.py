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
    by_id = {int(a.hittable): a for a in attrs}
    hittable = np.asarray(hittable).astype(np.int64)
    bu, bv, d = np.asarray(bu).astype(T), np.asarray(bv).astype(T), np.asarray(d).astype(T).reshape(-1, 3)
    N = len(hittable)
    n, ff, u, v = np.zeros((N, 3), T), np.zeros(N, bool), bu.copy(), bv.copy()
    tiny = T(np.finfo(np.float32).tiny)          # the device's test is made in f32

    def unit(x):
        return x / np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]).astype(T))[:, None]
    for h in np.unique(hittable):
        k = np.flatnonzero(hittable == h)
        P = np.asarray(tris[int(h)], dtype=np.float64).astype(T).reshape(3, 3)
        out = np.broadcast_to(unit(np.cross(P[1] - P[0], P[2] - P[0]).astype(T)[None, :]), (len(k), 3)).copy()
        a = by_id.get(int(h))
        if a is not None and a.flags & A.RT_TRI_NORMALS:
            vn = np.array([[a.n[i][c] for c in range(3)] for i in range(3)], dtype=np.float64)
            vn = (vn / np.linalg.norm(vn, axis=1, keepdims=True)).astype(T)
            w0 = (T(1.0) - bu[k] - bv[k]).astype(T)
            s = ((w0[:, None] * vn[0] + bu[k][:, None] * vn[1]).astype(T) + bv[k][:, None] * vn[2]).astype(T)
            l2 = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2]).astype(T)
            ok = (l2 >= tiny) & np.isfinite(l2)
            out[ok] = unit(s[ok])
        if a is not None and a.flags & A.RT_TRI_UVS:
            uv = np.array([[a.uv[i][c] for c in range(2)] for i in range(3)], dtype=np.float32).astype(T)
            u[k] = ((uv[0, 0] + bu[k] * (uv[1, 0] - uv[0, 0])).astype(T) + bv[k] * (uv[2, 0] - uv[0, 0])).astype(T)
            v[k] = ((uv[0, 1] + bu[k] * (uv[1, 1] - uv[0, 1])).astype(T) + bv[k] * (uv[2, 1] - uv[0, 1])).astype(T)
        front = (d[k, 0] * out[:, 0] + d[k, 1] * out[:, 1] + d[k, 2] * out[:, 2]).astype(T) < 0
        n[k], ff[k] = np.where(front[:, None], out, -out), front
    return n, ff, u, v
