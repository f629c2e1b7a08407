"""A/B of upload options on the GPU box: python3 scripts/gpu_ab_upload.py scene[,scene...] SETTING SETTING [SETTING ...]
(scenes: book1 | cornell | cornell_smoke | final). A SETTING is `default` or a comma-separated list of RT_LAYOUT_* flag names (the prefix may
be left out) and key=value pairs for lds_top_records, octant_axes, leaf_collapse, list_park_cost (RtUploadOptions) and tail_paths (RtParams),
e.g. `LISTS_AS_REFERENCE` or `NO_SHADE_TABLES_IN_LDS,tail_paths=1`. Every setting gets its own upload; the settings are rendered in turn,
twice over, and each frame is compared bit for bit with the first."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rta

OPTION_KEYS = {"lds_top_records": int, "octant_axes": int, "leaf_collapse": int, "list_park_cost": float}


def parse_setting(p, text):
    """SETTING -> (layout_flags, upload option kwargs, tail_paths)"""
    flags, opts, tail = 0, {}, 0
    for tok in ([] if text in ("", "default") else text.split(",")):
        key, _, value = tok.partition("=")
        if key == "tail_paths":
            tail = int(value)
        elif key in OPTION_KEYS:
            opts[key] = OPTION_KEYS[key](value)
        else:
            name = key if key.startswith("RT_LAYOUT_") else "RT_LAYOUT_" + key
            if not hasattr(p._abi, name):
                raise SystemExit(f"unknown setting {tok!r}")
            flags |= getattr(p._abi, name)
    return flags, opts, tail


if __name__ == "__main__":
    p = rta.load()
    settings = sys.argv[2:]
    if len(settings) < 2:
        raise SystemExit(__doc__)
    ctx = p.Context(0)
    for which in sys.argv[1].split(","):
        if which == "final":
            from PIL import Image
            hs = p.HostScene("final", 1, image=np.asarray(Image.open("tests/golden/earthmap_rgb.png").convert("RGB"))); W, H, spp = 800, 800, 200
        elif which in ("cornell", "cornell_smoke"):
            hs = p.HostScene(which, 0); W, H, spp = 600, 600, 500
        else:
            hs = p.HostScene("book1", 1); W, H, spp = 1200, 800, 500
        cam = hs.camera(W / H)
        ref = None
        for setting in settings * 2:
            flags, opts, tail = parse_setting(p, setting)
            scene = ctx.upload(hs.desc, flags, **opts)
            ctx.render(scene, cam, p.make_params(W, H, spp, tail_paths=tail))
            _, st = ctx.render(scene, cam, p.make_params(W, H, spp, flags=2, tail_paths=tail))     # per-kernel times (events around every launch)
            img, st0 = ctx.render(scene, cam, p.make_params(W, H, spp, tail_paths=tail))           # the production timing
            same = "" if ref is None else (" identical_to_first=%s" % bool(np.array_equal(ref, img)))
            if ref is None: ref = img
            print(which, setting, "extend_ms %.1f shade_ms %.1f drain_ms %.1f render_ms %.1f Msamples/s %.1f%s" % (st['extend_ms'], st['shade_ms'], st['drain_ms'], st0['render_ms'], W * H * spp / st0['render_ms'] / 1e3, same), flush=True)
            scene.close()
