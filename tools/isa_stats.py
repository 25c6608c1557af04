#!/usr/bin/env python3
"""Static picture of ONE render kernel instance (no GPU needed): registers, scratch, instruction mix.
usage: tools/isa_stats.py [--inst "false,true,false,6,false,true"] [--waves 7] [--keep out.s] [-- extra hipcc flags]
       tools/isa_stats.py --kernel "render_nee_kernel<false,7>"               (light sampling: <SCALAR, CULL>)
       tools/isa_stats.py --kernel "render_nested_kernel<false,true>"         (the nested grid: <COUNT, EXT>)
       tools/isa_stats.py --kernel "render_feature_kernel<false,7>"           (a feature pass: <SCALAR, CULL>)
       tools/isa_stats.py --kernel "render_env_kernel<false,7,true,false>"    (an environment map: <SCALAR, CULL, NEE, AOV>)
       tools/isa_stats.py --kernel "render_media_kernel<false,7>" -- -DRT_MEDIA_WAVES_PER_SIMD=6    (media: <SCALAR, CULL>)
       tools/isa_stats.py --media-nee "false,7" -- -DRT_MEDIA_NEE_WAVES_PER_SIMD=5     (light sampling in media: media_nee_kernel<SCALAR, CULL>)
       tools/isa_stats.py --kernel "render_motion_kernel<false,7>"            (moving spheres: <SCALAR, CULL>)
       tools/isa_stats.py --kernel "trace_kernel<false,7>"                    (ray queries: <SCALAR, CULL>)
       tools/isa_stats.py --kernel "alpha_kernel<1,false,0>"                  (a scene with alpha masks: <FAMILY, SCALAR, CULL>, csrc/alpha_kernel.h)
       tools/isa_stats.py --kernel "camera_kernel<16,false,7>"                (a non-perspective camera: <FAMILY, SCALAR, CULL>, csrc/camera_kernel.h)
--inst ARGS is short for --kernel "render_kernel<ARGS>"; the default instance is the headline kernel (sphere-only x-z grid walk,
variant 0 -> 2 on RTIOW).  The families whose register budget is not --waves take theirs after "--":
-DRT_NEE_WAVES_PER_SIMD=N (render_nee_kernel, render_env_kernel with NEE), -DRT_MEDIA_WAVES_PER_SIMD=N, -DRT_MEDIA_NEE_WAVES_PER_SIMD=N, -DRT_MOTION_WAVES_PER_SIMD=N,
and the two big-workgroup instances of render_kernel (<false,true,false,6,false,true> and <false,true,false,5,false,true>, csrc/kernels.h)
-DRT_BIG_WAVES_PER_SIMD=N (default 8) with -DRT_BIG_WAVES=n waves per workgroup; -DRT_BIG_GROUPS=0 gives them the 4-wave shape and --waves."""
import argparse, collections, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the translation unit of a kernel template (render_nee_kernel, render_nested_kernel and render_feature_kernel live in render_kernel.hip too)
SOURCES = {"render_kernel": "render_kernel.hip", "render_env_kernel": "render_env.hip", "render_media_kernel": "render_media.hip",
           "render_motion_kernel": "render_motion.hip", "trace_kernel": "trace.hip", "alpha_kernel": "alpha_kernel.hip",
           "camera_kernel": "camera_kernel.hip", "media_nee_kernel": "media_nee_kernel.hip"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inst", default="false,true,false,6,false,true", help="template arguments of a render_kernel instance")
    ap.add_argument("--kernel", default=None, help="a whole template-id instead of --inst, e.g. 'render_media_kernel<false,7>'")
    ap.add_argument("--media-nee", default=None, help="short for --kernel 'media_nee_kernel<ARGS>', e.g. 'false,7'")
    ap.add_argument("--waves", type=int, default=7)
    ap.add_argument("--keep", default=None)
    ap.add_argument("extra", nargs="*")
    a = ap.parse_args()
    if a.media_nee:
        a.kernel = "media_nee_kernel<%s>" % a.media_nee
    name, args = re.fullmatch(r"(\w+)<(.*)>", a.kernel or "render_kernel<%s>" % a.inst).groups()
    src = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "csrc", SOURCES.get(name, SOURCES["render_kernel"]))
    out = a.keep or os.path.join(tempfile.gettempdir(), "rtmi_isa_%d.s" % os.getpid())
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fno-slp-vectorize", "-DRT_WAVES_PER_SIMD=%d" % a.waves, "-DRT_GROUP=4", "-DRT_ISA_ONLY=%s<%s>" % (name, args),
           "--offload-device-only", "-S", "-o", out, src] + a.extra
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    body = text[text.index(name):]
    meta = {}
    for key in ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size", "accum_offset"):
        m = re.search(r"amdhsa_%s (\d+)" % key, text)
        meta[key] = int(m.group(1)) if m else None
    for key in ("sgpr_spill_count", "vgpr_spill_count"):
        m = re.search(r"\.%s:\s+(\d+)" % key, text)
        meta[key] = int(m.group(1)) if m else None
    mix = collections.Counter()
    names = collections.Counter()
    for line in body.splitlines():
        m = re.match(r"\s+([a-z_0-9]+)\s", line + " ")
        if not m:
            continue
        op = m.group(1)
        if op.startswith("v_"):
            mix["valu"] += 1
        elif op.startswith("s_cbranch") or op == "s_branch":
            mix["branch"] += 1
        elif op.startswith("s_waitcnt") or op == "s_nop":
            mix["wait/nop"] += 1
        elif op.startswith("s_"):
            mix["salu"] += 1
        elif op.startswith("ds_"):
            mix["lds"] += 1
        elif op.startswith("scratch_"):
            mix["scratch"] += 1
        elif op.startswith("global_") or op.startswith("flat_") or op.startswith("buffer_"):
            mix["vmem"] += 1
        else:
            continue
        names[op] += 1
    own = dict(re.findall(r"-D(RT_\w+_WAVES_PER_SIMD)=(\d+)", " ".join(a.extra)))  # a family's own budget, where it was given
    if name == "render_kernel":
        print("instance <%s> at %d waves/SIMD" % (args, a.waves))
    elif name == "render_nee_kernel":
        print("render_nee_kernel <%s> at %s waves/SIMD" % (args, own.get("RT_NEE_WAVES_PER_SIMD", "the default")))
    elif name == "render_env_kernel":
        print("render_env_kernel <%s> at %d waves/SIMD (light sampling: %s)" % (args, a.waves, own.get("RT_NEE_WAVES_PER_SIMD", "the default")))
    elif name == "media_nee_kernel":
        print("media_nee_kernel <%s> at %s waves/SIMD" % (args, own.get("RT_MEDIA_NEE_WAVES_PER_SIMD", own.get("RT_NEE_WAVES_PER_SIMD", "the default"))))
    elif name in ("render_media_kernel", "render_motion_kernel"):
        print("%s <%s> at %s waves/SIMD" % (name, args, own.get("RT_%s_WAVES_PER_SIMD" % name.split("_")[1].upper(), a.waves)))
    else:
        print("%s <%s> at %d waves/SIMD" % (name, args, a.waves))
    print("  registers:", meta)
    print("  static instruction mix:", dict(mix), "total", sum(mix.values()))
    hot = ["v_readlane_b32", "v_writelane_b32", "v_mov_b32_e32", "v_cndmask_b32_e32", "v_cndmask_b32_e64", "scratch_load_dword",
           "scratch_store_dword", "ds_bpermute_b32", "v_mul_hi_u32", "v_mul_lo_u32", "v_sqrt_f32_e32", "v_rcp_f32_e32"]
    print("  selected:", {k: names[k] for k in hot if names[k]})
    if not a.keep:
        os.unlink(out)


if __name__ == "__main__":
    main()
