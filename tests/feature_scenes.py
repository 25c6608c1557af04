"""What the scene modules of the feature suites share ({alpha,bump,glass,glossy,noise,normal_map,quad,pbr,mesh_light,
analytic_light}_scenes.py): the family bits of rt_stats.kernel_variant, a case's seed and inputs, and the step that makes a
twin plain.  A module keeps its builders, CASES, MISTAKES and check_contents, and binds family / seed_of / inputs with
bindings()."""
import media_scenes as MS
import motion_scenes as MO
import nee_scenes as NS
import ref64 as R

NEE, ENV, MEDIA, MOTION = 256, 1024, MS.MEDIA, MO.MOTION
FAMILIES = NEE | ENV | MEDIA | MOTION


def bindings(entry):
    """(family, seed_of, inputs) of a module whose entry(name)[0] holds the family bits the kernel must report on the case.
    seed_of(name): the media and motion cases use their families' seed; inputs(rtmi, name): (uniforms, shutter times or None)
    of the case's 48 x 27 x 13 samples"""
    def family(name):
        return entry(name)[0]

    def seed_of(name):
        return NS.REF_SEED if not family(name) & (MEDIA | MOTION) else MS.REF_SEED

    def inputs(rtmi, name):
        words = R.uniforms(rtmi, seed_of(name), NS.REF_W, NS.REF_H, 0, NS.REF_K, NS.REF_DRAWS)
        shutter = MO.shutter_times(rtmi, seed_of(name), NS.REF_W, NS.REF_H, 0, NS.REF_K) if family(name) == MOTION else None
        return words, shutter
    return family, seed_of, inputs


def cleared(sc, analytic_lights=True):
    """the scene as the plain kernel renders it: light sampling off, its environment, media, movers and (unless the caller keeps
    them: without light sampling they light nothing) analytic lights cleared.  Clearing what a scene does not have changes nothing"""
    sc.set_light_sampling(False)
    sc.set_environment(None)
    sc.clear_media()
    sc.clear_moving_spheres()
    if analytic_lights:
        sc.clear_analytic_lights()
    return sc
