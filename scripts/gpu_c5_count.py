"""Config 5 stand-in at 2048x2048 with counters: tests per segment. usage: gpu_c5_count.py [spp [SETTING]]
(SETTING: upload options and tail_paths, as in gpu_ab_upload.py)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rta
from gpu_ab_upload import parse_setting
p = rta.load()
flags, opts, tail = parse_setting(p, sys.argv[2] if len(sys.argv) > 2 else "default")
ctx = p.Context(0)
hs = p.HostScene("big_sah", 5, 1000000, 512)
scene = ctx.upload(hs.desc, flags, **opts)
cam = hs.camera(1.0)
W = H = 2048; spp = int(sys.argv[1]) if len(sys.argv) > 1 else 16
for md in (16,):
    t = time.time(); img, st = ctx.render(scene, cam, p.make_params(W, H, spp, flags=1, max_depth=md, tail_paths=tail)); dt = time.time() - t
    print(os.environ.get("RT_HIP_LIB", "default").split("_")[-1], "max_depth", md, "%.1f ms" % (dt * 1e3), "segments", st["segments"], "node tests/seg %.2f" % (st["node_tests"] / st["segments"]),
          "prim/seg", [round(x / st["segments"], 3) for x in st["prim_tests"]], flush=True)
