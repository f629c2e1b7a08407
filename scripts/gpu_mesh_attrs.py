"""What smooth shading costs on one MI355X: config 5's procedural mesh (the 512 x 256 torus, 262 144 triangles, Metal, on the ground rect
under the sky) rendered flat and with generated vertex normals, in Msamples/s:  python scripts/gpu_mesh_attrs.py [result.json]
(the figures are printed; with a file name they are written there as JSON too).
The mesh is written into the RtHittable / RtTriangleAttrs arrays with numpy (a quarter of a million SceneBuilder calls would take longer
than the renders)."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rta

p = rta.load()
A = p._abi
NU, NV, R0, r0 = 512, 256, 30.0, 10.0
W = H = 1024
SPP = 512

b = p.SceneBuilder(background=(0.5, 0.7, 1.0), background_mode=A.RT_BG_SKY_GRADIENT, bvh_builder=A.RT_BVH_SAH)
ground = b.xz_rect(-600, 600, -600, 600, 0, b.lambertian((0.5, 0.5, 0.5)))
gold = b.metal((0.8, 0.7, 0.3), 0.05)
iu, iv = np.meshgrid(np.arange(NU + 1), np.arange(NV + 1), indexing="ij")
a, c = 2 * np.pi * (iu % NU) / NU, 2 * np.pi * (iv % NV) / NV
P = np.stack([(R0 + r0 * np.cos(c)) * np.cos(a), 12 + r0 * np.sin(c), (R0 + r0 * np.cos(c)) * np.sin(a)], axis=-1)
Nrm = np.stack([np.cos(c) * np.cos(a), np.sin(c), np.cos(c) * np.sin(a)], axis=-1)            # the torus' own normal at every vertex
quad = lambda X: (X[:-1, :-1], X[1:, :-1], X[1:, 1:], X[:-1, 1:])
p00, p10, p11, p01 = quad(P)
n00, n10, n11, n01 = quad(Nrm)
tris = np.concatenate([np.stack([p00, p10, p11], axis=2).reshape(-1, 9), np.stack([p00, p11, p01], axis=2).reshape(-1, 9)])
nrms = np.concatenate([np.stack([n00, n10, n11], axis=2).reshape(-1, 9), np.stack([n00, n11, n01], axis=2).reshape(-1, 9)])
n_tri = len(tris)
first = len(b.hittables)                      # the ground rect is record 0; the triangles follow, then the BVH over all of it
hit_t = np.dtype([("kind", "<i4"), ("material", "<i4"), ("first_child", "<i4"), ("n_children", "<i4"), ("p", "<f8", 10)])
att_t = np.dtype([("hittable", "<i4"), ("flags", "<u4"), ("n", "<f4", 9), ("uv", "<f4", 6)])
assert hit_t.itemsize == C.sizeof(A.RtHittable) and att_t.itemsize == C.sizeof(A.RtTriangleAttrs)
hits = np.zeros(first + n_tri + 1, hit_t)
for k in range(first):
    h = b.hittables[k]
    hits[k] = (h.kind, h.material, h.first_child, h.n_children, list(h.p))
hits["kind"][first:first + n_tri], hits["material"][first:first + n_tri] = A.RT_HIT_TRIANGLE, gold
hits["first_child"][first:first + n_tri] = -1
hits["p"][first:first + n_tri, :9] = tris
children = np.concatenate([[ground], np.arange(first, first + n_tri)]).astype(np.int32)
hits[first + n_tri] = (A.RT_HIT_BVH, -1, 0, len(children), [0.0] * 10)
attrs = np.zeros(n_tri, att_t)
attrs["hittable"], attrs["flags"], attrs["n"] = np.arange(first, first + n_tri), A.RT_TRI_NORMALS, nrms
desc = b.desc(ground)
desc.hittables, desc.n_hittables = hits.ctypes.data_as(C.POINTER(A.RtHittable)), len(hits)
desc.children, desc.n_children = children.ctypes.data_as(C.POINTER(C.c_int32)), len(children)
desc.world = first + n_tri
attr_arr = (A.RtTriangleAttrs * n_tri).from_buffer(attrs)
cam = p.camera_new((130, 40, 60), (0, 5, 0), (0, 1, 0), 30.0, W / H, 0.0, 10.0, 0.0, 0.0)

ctx = p.Context(0)
out = {"mesh": f"torus {NU} x {NV}: {n_tri} triangles, Metal fuzz 0.05, SAH", "width": W, "height": H, "spp": SPP}
for tag, at in (("flat", None), ("smooth", attr_arr)):
    info = p.compile_info(desc, triangle_attrs=at)
    t = time.time(); scene = ctx.upload(desc, triangle_attrs=at); t_up = time.time() - t
    ctx.render(scene, cam, p.make_params(W, H, SPP))
    best = None
    for _ in range(3):
        t = time.time(); img, st = ctx.render(scene, cam, p.make_params(W, H, SPP, flags=A.RT_FLAG_TIMING)); dt = time.time() - t
        if best is None or dt < best[0]:
            best = (dt, st)
    dt, st = best
    out[tag] = dict(features=info["features"], n_tri_attrs=info["n_tri_attrs"], seconds=round(dt, 4), msamples_per_s=round(W * H * SPP / dt / 1e6, 1), upload_s=round(t_up, 2),
                    extend_ms=round(st["extend_ms"], 2), shade_ms=round(st["shade_ms"], 2), segments_per_sample=round(st["segments"] / st["samples"], 3),
                    scene_bytes=st["scene_bytes"], mean_level=round(float(img.mean()) / SPP, 5))
    print(tag, out[tag], flush=True)
    scene.close()
print(json.dumps(out))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
