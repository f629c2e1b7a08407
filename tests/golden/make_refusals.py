"""The table of refused calls behind tests/golden/refusals.json: every options struct of include/rt_hip.h that a host-only check
function reads — struct_bytes 0, struct_bytes = sizeof - 8, an unknown flag bit, the first value-range refusal of the function — and every
device entry point called with ctx null. No call here needs a device. Run as a script it records (return code, rt_last_error(NULL)) of
every case; tests/test_refusals_host.py replays cases() against the built library and asserts both, byte for byte."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "refusals.json")


def cases(pkg):
    """[(name, thunk)]: thunk() makes the call and returns its code."""
    A, lib = pkg._abi, pkg.lib()
    ref = lambda o: C.byref(o) if o is not None else None
    prm = lambda **kw: pkg.make_params(64, 40, 4, **kw)
    out = []

    def header(fn_name, T, call, flag_field="flags", unknown=1 << 9):
        """the three header cases of struct T; call(o) passes the struct to the function"""
        def make(**kw):
            o = T()
            o.struct_bytes = C.sizeof(T)
            for k, v in kw.items():
                setattr(o, k, v)
            return o
        out.append((f"{fn_name}/{T.__name__}.struct_bytes=0", lambda: call(make(struct_bytes=0))))
        out.append((f"{fn_name}/{T.__name__}.struct_bytes=sizeof-8", lambda: call(make(struct_bytes=C.sizeof(T) - 8))))
        if flag_field:
            out.append((f"{fn_name}/{T.__name__}.{flag_field}=unknown", lambda: call(make(**{flag_field: unknown}))))
        return make

    # rt_pass_check
    call_p = lambda o, p=None: lib.rt_pass_check(C.byref(p or prm()), ref(o), None)
    make_p = header("rt_pass_check", A.RtPassOptions, call_p)
    out.append(("rt_pass_check/options=null", lambda: call_p(None)))
    out.append(("rt_pass_check/first_sample+spp=2^32", lambda: call_p(make_p(first_sample=0xFFFFFFFF, frame_samples=0xFFFFFFFF))))
    out.append(("rt_pass_check/frame_samples<end", lambda: call_p(make_p(first_sample=4, frame_samples=6))))
    out.append(("rt_pass_check/params.flags=unknown", lambda: call_p(make_p(frame_samples=4), prm(flags=1 << 9))))
    # rt_adaptive_check (the struct has no flags word)
    call_a = lambda o, first=0, frame=64: lib.rt_adaptive_check(C.byref(prm()), ref(o), first, frame)
    make_a = header("rt_adaptive_check", A.RtAdaptiveOptions, call_a, flag_field=None)
    out.append(("rt_adaptive_check/options=null", lambda: call_a(None)))
    out.append(("rt_adaptive_check/rel_error<0", lambda: call_a(make_a(min_samples=2, rel_error=-1.0))))
    out.append(("rt_adaptive_check/min_samples<2", lambda: call_a(make_a(min_samples=1, rel_error=0.01))))
    # rt_ray_query_check
    call_q = lambda o, n=1: lib.rt_ray_query_check(ref(o), n)
    make_q = header("rt_ray_query_check", A.RtRayQueryOptions, call_q)
    out.append(("rt_ray_query_check/flags=RT_FLAG_COUNTERS", lambda: call_q(make_q(flags=A.RT_FLAG_COUNTERS))))
    out.append(("rt_ray_query_check/n_rays=2^32", lambda: call_q(make_q(), 1 << 32)))
    out.append(("rt_ray_query_check/options=null,n_rays=2^40", lambda: call_q(None, 1 << 40)))
    # rt_radiance_check
    call_r = lambda o, n=1: lib.rt_radiance_check(ref(o), n)
    good = dict(samples=4, max_depth=50)
    make_r = header("rt_radiance_check", A.RtRadianceOptions, lambda o: call_r(o), unknown=2)
    out.append(("rt_radiance_check/options=null", lambda: call_r(None)))
    out.append(("rt_radiance_check/render_flags=RT_FLAG_COUNTERS", lambda: call_r(make_r(render_flags=A.RT_FLAG_COUNTERS, **good))))
    out.append(("rt_radiance_check/nan_policy=2", lambda: call_r(make_r(nan_policy=2, **good))))
    out.append(("rt_radiance_check/samples=0", lambda: call_r(make_r(max_depth=50))))
    out.append(("rt_radiance_check/first_stream+n_rays=2^32", lambda: call_r(make_r(first_stream=0xFFFFFFFF, **good), 1)))
    # rt_features_check
    call_f = lambda o, p=None: lib.rt_features_check(C.byref(p or prm()), ref(o))
    make_f = header("rt_features_check", A.RtFeatureOptions, call_f, unknown=2)
    out.append(("rt_features_check/options=null", lambda: call_f(None)))
    out.append(("rt_features_check/first_sample+spp=2^32", lambda: call_f(make_f(first_sample=0xFFFFFFFF))))
    out.append(("rt_features_check/params.flags=RT_FLAG_COUNTERS", lambda: call_f(make_f(), prm(flags=A.RT_FLAG_COUNTERS))))
    # rt_feature_moments_check: the options as above, then the buffers record (it has no flags word)
    fopt = make_f()
    mcall = lambda o, b: lib.rt_feature_moments_check(C.byref(prm()), ref(o), ref(b))
    mbuf = A.RtFeatureMomentBuffers(C.sizeof(A.RtFeatureMomentBuffers))
    header("rt_feature_moments_check", A.RtFeatureOptions, lambda o: mcall(o, mbuf), unknown=2)
    out.append(("rt_feature_moments_check/first_sample+spp=2^32", lambda: mcall(make_f(first_sample=0xFFFFFFFF), mbuf)))
    header("rt_feature_moments_check", A.RtFeatureMomentBuffers, lambda b: mcall(fopt, b), flag_field=None)
    out.append(("rt_feature_moments_check/buffers=null", lambda: mcall(fopt, None)))
    # rt_denoise_check and its guided kin (RtDenoiseOptions has no flags word)
    call_d = lambda o, w=64, h=40: lib.rt_denoise_check(w, h, ref(o))
    make_d = header("rt_denoise_check", A.RtDenoiseOptions, call_d, flag_field=None)
    out.append(("rt_denoise_check/width=0", lambda: call_d(None, 0, 40)))
    out.append(("rt_denoise_check/window_radius=17", lambda: call_d(make_d(window_radius=17))))
    out.append(("rt_denoise_check/strength<0", lambda: call_d(make_d(strength=-1.0))))
    for fn_name, T, fs_low, r_high in (("rt_denoise_guided_check", A.RtDenoiseGuide, 0, 11), ("rt_denoise_guided_moments_check", A.RtDenoiseGuideMoments, 1, 9)):
        fn = getattr(lib, fn_name)
        gcall = lambda o, g, fn=fn: fn(64, 40, ref(o), ref(g))
        some = lambda T=T, **kw: T(C.sizeof(T), kw.pop("feature_samples", 4), 16, **kw)     # albedo_sum = a non-null address the check never reads
        header(fn_name, A.RtDenoiseOptions, lambda o, gcall=gcall, some=some: gcall(o, some()), flag_field=None)
        make_g = header(fn_name, T, lambda g, gcall=gcall: gcall(None, g), flag_field=None)
        out.append((f"{fn_name}/guide=null", lambda gcall=gcall: gcall(None, None)))
        out.append((f"{fn_name}/window_radius={r_high}", lambda gcall=gcall, some=some, r=r_high: gcall(make_d(window_radius=r), some())))
        out.append((f"{fn_name}/feature_samples={fs_low}", lambda gcall=gcall, some=some, k=fs_low: gcall(None, some(feature_samples=k))))
        out.append((f"{fn_name}/no plane", lambda gcall=gcall, make_g=make_g: gcall(None, make_g(feature_samples=4))))
        out.append((f"{fn_name}/sigma_albedo<0", lambda gcall=gcall, some=some: gcall(None, some(sigma_albedo=-1.0))))
    # every device entry point, ctx null
    for name, n_args, ints in (("rt_render", 6, ()), ("rt_render_device", 6, ()), ("rt_render_pass", 8, ()), ("rt_render_pass_device", 8, ()),
                               ("rt_render_pass_pixels_device", 11, (6,)), ("rt_adaptive_select", 10, (3, 4)), ("rt_resolve_counts_device", 6, (3, 4)),
                               ("rt_resolve_device", 6, (2, 3, 4)),
                               ("rt_trace_rays", 7, (4,)), ("rt_trace_rays_device", 7, (4,)), ("rt_occluded_rays", 7, (4,)), ("rt_occluded_rays_device", 7, (4,)),
                               ("rt_sample_lights", 7, (4,)), ("rt_sample_lights_device", 7, (4,)), ("rt_radiance_rays", 9, (4,)), ("rt_radiance_rays_device", 9, (4,)),
                               ("rt_render_features_device", 7, ()), ("rt_render_feature_moments_device", 7, ()),
                               ("rt_denoise_device", 9, (2, 3, 6)), ("rt_denoise_guided_device", 10, (3, 4, 7)), ("rt_denoise_guided_moments_device", 10, (3, 4, 7))):
        args = [0 if k in ints else None for k in range(n_args)]
        out.append((f"{name}/ctx=null", lambda fn=getattr(lib, name), args=args: fn(*args)))
    return out


def record(pkg):
    """[{case, code, error}] of the library `pkg` has loaded"""
    rows = []
    for name, thunk in cases(pkg):
        pkg.lib().rt_output_floats(None, None)          # "null argument": a case that sets no message of its own does not inherit the last one's
        code = thunk()
        rows.append({"case": name, "code": int(code), "error": pkg.lib().rt_last_error(None).decode()})
    return rows


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import rta
    rows = record(rta.load())
    assert all(r["code"] != 0 for r in rows), [r["case"] for r in rows if r["code"] == 0]
    with open(FIXTURE, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    print(len(rows), "refusals ->", FIXTURE)
