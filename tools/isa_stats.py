#!/usr/bin/env python3
"""Static picture of ONE render_kernel instance (no GPU needed): registers, scratch, instruction mix.
usage: tools/isa_stats.py [--inst "false,true,false,6,false,true"] [--waves 7] [--keep out.s] [-- extra hipcc flags]
       tools/isa_stats.py --nee "false,7" [--nee-waves 6]     (a light-sampling kernel: render_nee_kernel<SCALAR, CULL>)
       tools/isa_stats.py --nested "false,true"               (a nested-grid kernel: render_nested_kernel<COUNT, EXT>)
       tools/isa_stats.py --aov "false,7"                     (a feature kernel: render_feature_kernel<SCALAR, CULL>)
       tools/isa_stats.py --env "false,7,true,false"          (an environment kernel: render_env_kernel<SCALAR, CULL, NEE, AOV>)
       tools/isa_stats.py --media "false,7" [--media-waves 6] (a media kernel: render_media_kernel<SCALAR, CULL>)
       tools/isa_stats.py --motion "false,7" [--motion-waves 6] (a motion kernel: render_motion_kernel<SCALAR, CULL>)
The default instance is the headline kernel (sphere-only x-z grid walk, variant 0 -> 2 on RTIOW)."""
import argparse, collections, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "csrc", "render_kernel.hip")
SRC_ENV = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "csrc", "render_env.hip")
SRC_MEDIA = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "csrc", "render_media.hip")
SRC_MOTION = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "csrc", "render_motion.hip")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inst", default="false,true,false,6,false,true")
    ap.add_argument("--waves", type=int, default=7)
    ap.add_argument("--nee", default=None, help="SCALAR,CULL of a render_nee_kernel instance instead of --inst")
    ap.add_argument("--nee-waves", type=int, default=None)
    ap.add_argument("--nested", default=None, help="COUNT,EXT of a render_nested_kernel instance instead of --inst")
    ap.add_argument("--aov", default=None, help="SCALAR,CULL of a render_feature_kernel instance instead of --inst")
    ap.add_argument("--env", default=None, help="SCALAR,CULL,NEE,AOV of a render_env_kernel instance instead of --inst")
    ap.add_argument("--media", default=None, help="SCALAR,CULL of a render_media_kernel instance instead of --inst")
    ap.add_argument("--media-waves", type=int, default=None)
    ap.add_argument("--motion", default=None, help="SCALAR,CULL of a render_motion_kernel instance instead of --inst")
    ap.add_argument("--motion-waves", type=int, default=None)
    ap.add_argument("--keep", default=None)
    ap.add_argument("extra", nargs="*")
    a = ap.parse_args()
    out = a.keep or os.path.join(tempfile.gettempdir(), "rtmi_isa_%d.s" % os.getpid())
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fno-slp-vectorize", "-DRT_WAVES_PER_SIMD=%d" % a.waves, "-DRT_GROUP=4",
           ("-DRT_ISA_ONLY_MOTION=" + a.motion) if a.motion else
           ("-DRT_ISA_ONLY_MEDIA=" + a.media) if a.media else
           ("-DRT_ISA_ONLY_ENV=" + a.env) if a.env else
           ("-DRT_ISA_ONLY_AOV=" + a.aov) if a.aov else
           ("-DRT_ISA_ONLY_NEE=" + a.nee) if a.nee else (("-DRT_ISA_ONLY_NESTED=" + a.nested) if a.nested else ("-DRT_ISA_ONLY=" + a.inst))]
    if (a.nee or a.env) and a.nee_waves:
        cmd.append("-DRT_NEE_WAVES_PER_SIMD=%d" % a.nee_waves)
    if a.media and a.media_waves:
        cmd.append("-DRT_MEDIA_WAVES_PER_SIMD=%d" % a.media_waves)
    if a.motion and a.motion_waves:
        cmd.append("-DRT_MOTION_WAVES_PER_SIMD=%d" % a.motion_waves)
    cmd += [
           "--offload-device-only", "-S", "-o", out, SRC_MOTION if a.motion else SRC_MEDIA if a.media else SRC_ENV if a.env else SRC] + a.extra
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    body = text[text.index("render_motion_kernel" if a.motion else "render_media_kernel" if a.media else "render_env_kernel" if a.env else "render_feature_kernel" if a.aov else
                           "render_nee_kernel" if a.nee else ("render_nested_kernel" if a.nested else "render_kernel")):]
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
    if a.motion:
        print("render_motion_kernel <%s> at %s waves/SIMD" % (a.motion, a.motion_waves or a.waves))
    elif a.media:
        print("render_media_kernel <%s> at %s waves/SIMD" % (a.media, a.media_waves or a.waves))
    elif a.env:
        print("render_env_kernel <%s> at %d waves/SIMD (light sampling: %s)" % (a.env, a.waves, a.nee_waves or "the default"))
    elif a.aov:
        print("render_feature_kernel <%s> at %d waves/SIMD" % (a.aov, a.waves))
    elif a.nested:
        print("render_nested_kernel <%s> at %d waves/SIMD" % (a.nested, a.waves))
    elif a.nee:
        print("render_nee_kernel <%s> at %s waves/SIMD" % (a.nee, a.nee_waves or "the default"))
    else:
        print("instance <%s> at %d waves/SIMD" % (a.inst, a.waves))
    print("  registers:", meta)
    print("  static instruction mix:", dict(mix), "total", sum(mix.values()))
    hot = ["v_readlane_b32", "v_writelane_b32", "v_mov_b32_e32", "v_cndmask_b32_e32", "v_cndmask_b32_e64", "scratch_load_dword",
           "scratch_store_dword", "ds_bpermute_b32", "v_mul_hi_u32", "v_mul_lo_u32", "v_sqrt_f32_e32", "v_rcp_f32_e32"]
    print("  selected:", {k: names[k] for k in hot if names[k]})
    if not a.keep:
        os.unlink(out)


if __name__ == "__main__":
    main()
