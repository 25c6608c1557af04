/*
 * rtmi.h -- C ABI of librtmi.so, the MI355X-native per-pixel path tracer.
 *
 * This is the drop-in boundary for the reference's hot path
 *     scene JSON  ->  render kernel  ->  float framebuffer  ->  PPM
 * Every entry point names the reference interface it replaces.  Paths are
 * relative to the reference checkout (gpu-version/ = CUDA renderer whose
 * interface is kept, cmake-cpu-version/ = CPU renderer whose ray_color
 * semantics are followed).
 *
 * Conventions
 *   - plain C: pointers, sizes, POD structs; no C++/torch/HIP types.
 *   - every function that can fail returns an rt_status (0 = RT_OK); the text
 *     of the last failure on the calling thread is at rt_last_error().
 *     The library never calls exit() (the reference does: rtweekend.cuh:41-53).
 *   - framebuffer layout is the reference's: rgb_sum[(y*W + x)*3 + c] holds the
 *     SUM over samples (not the mean), fp32, row y = 0 is the BOTTOM row
 *     (gpu-version/main.cu:76-78,102-104); division by spp and gamma are the
 *     writer's job (gpu-version/color.cuh:70-95).
 *   - there is no CPU fallback: rt_render_* fail with RT_ERR_HIP when no
 *     gfx950 device / runtime is usable.
 */
#ifndef RTMI_H
#define RTMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTMI_ABI_VERSION 3

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_ARG = 1,     /* null / out-of-range argument                      */
    RT_ERR_IO = 2,      /* file cannot be read / written                     */
    RT_ERR_JSON = 3,    /* malformed JSON text                               */
    RT_ERR_SCENE = 4,   /* well-formed JSON, invalid scene (unknown type...) */
    RT_ERR_HIP = 5,     /* HIP runtime / device error                        */
    RT_ERR_LIMIT = 6    /* an explicitly requested LDS-table kernel variant cannot hold the scene,
                           or the work-item count overflows (the default variant has no scene limit) */
} rt_status;

/* ---- table records (what the scene flattens to; also what the checker in
 *      tests/ reads back through rt_scene_get_*) ------------------------- */

/* gpu-version/rtweekend.cuh:70-91 (enum class class_type) */
typedef enum rt_prim_type {
    RT_PRIM_SPHERE = 0,   /* object.cuh:40-94   f = {cx,cy,cz,radius}        */
    RT_PRIM_XY_RECT = 1,  /* object.cuh:96-132  f = {x0,x1,y0,y1,k}          */
    RT_PRIM_XZ_RECT = 2,  /* object.cuh:134-164 f = {x0,x1,z0,z1,k}          */
    RT_PRIM_YZ_RECT = 3,  /* object.cuh:166-197 f = {y0,y1,z0,z1,k}          */
    RT_PRIM_CYLINDER = 4, /* object.cuh:216-297 f = {radius,zmin,zmax}, m/m_inv */
    RT_PRIM_TRIANGLE = 5, /* taichi-version/hittable.py:38-71, 95-110: m[0..8] = v1, v2, v3; m[9..11] = the unit
                             normal (v2-v1)x(v3-v1) / |..|; m_inv[0..5] = texture coordinates u1, u2, u3 (2 each);
                             the unit vertex normals of smooth shading: f[0..2] = n1, f[3..5] = n2,
                             m_inv[6..8] = n3 -- all nine words zero: a flat triangle; m_inv[9..11] = 0 */
    RT_PRIM_QUAD = 6      /* a parallelogram (the model: csrc/rt_quad.h) with corner Q and edges u, v -- the corners
                             Q, Q + u, Q + u + v, Q + v: m[0..8] = Q, u, v; and, derived in fp64 from those fp32 values and
                             rounded once, with c = u x v and w = c / (c.c): m[9..11] = the outward unit normal n = c / |c|,
                             m_inv[0..2] = A = v x w, m_inv[3..5] = B = w x u; f and m_inv[6..11] = 0.  The hit: den = n.d
                             (zero or not finite: a miss), t = n.(Q - o) / den, p = o + t d, a = A.(p - Q), b = B.(p - Q),
                             a hit iff both lie in [0, 1]; the hit record's (u, v) = (a, b), front = den < 0 */
} rt_prim_type;

typedef enum rt_mat_type {
    RT_MAT_LAMBERTIAN = 0,    /* material.cuh:28-56   tex = albedo texture   */
    RT_MAT_METAL = 1,         /* material.cuh:58-75   albedo, fuzz (<=1)     */
    RT_MAT_DIELECTRIC = 2,    /* material.cuh:89-159  ir                     */
    RT_MAT_DIFFUSE_LIGHT = 3, /* material.cuh:161-182 tex = emission texture */
    /* glossy materials: a GGX microfacet lobe.  They reuse the record's fields:                      */
    RT_MAT_ROUGH_METAL = 4,   /* albedo = F0, fuzz = roughness in [0, 1]                                       */
    RT_MAT_PLASTIC = 5,       /* texture = body colour, fuzz = roughness in [0, 1], ir = the coat's index (> 1) */
    RT_MAT_ROUGH_GLASS = 6,   /*  ir = the index (> 1), fuzz = roughness in [0, 1], albedo = the absorption
                                 coefficient sigma per unit world length (each >= 0), texture = -1              */
    RT_MAT_PBR = 7            /*  metallic-roughness: texture = base colour, albedo[0] = the metallic factor,
                                 fuzz = the roughness factor (both in [0, 1]), ir = the coat's index (> 1), albedo[1..2] = 0;
                                 its map: rt_scene_set_pbr_map                                                   */
} rt_mat_type;

typedef enum rt_tex_type {
    RT_TEX_SOLID = 0,   /* texture.cuh:14-31  c0                             */
    RT_TEX_CHECKER = 1, /* texture.cuh:33-57  c0 = even, c1 = odd            */
    RT_TEX_IMAGE = 2,   /* taichi-version/material.py:137-144: texel lookup by the hit record's (u, v);
                           c0 = {image index, rows, columns} as floats (exact: small integers) */
    RT_TEX_NOISE = 3    /* a procedural solid texture: c0 + s (c1 - c0), s in [0, 1] from lattice noise at the
                           hit point; the parameters (rt_noise) live beside the texture table: rt_scene_get_noise */
} rt_tex_type;

/* Noise textures (the model: csrc/rt_noise.h).  Gradient noise n(q, seed) on the hashed integer lattice, summed over
 * `octaves` octaves of doubling frequency and halving amplitude from `scale` x the world-space hit point p:
 *   S = sum 2^-o n(2^o scale p, seed + o),  A = the same sum over |n|
 *   fbm: s = clamp(0.5 + 0.5 S, 0, 1)    turbulence: s = min(1, A)    marble: s = 0.5 + 0.5 sin(scale p[axis] + distortion A) */
typedef enum rt_noise_style {
    RT_NOISE_STYLE_FBM = 0,
    RT_NOISE_STYLE_TURBULENCE = 1,
    RT_NOISE_STYLE_MARBLE = 2
} rt_noise_style;

typedef struct rt_noise {
    int32_t style, octaves; /* rt_noise_style; 1..8                                                      */
    uint32_t seed;
    int32_t axis;           /* marble alone: 0 = x, 1 = y, 2 = z (the other styles store 0)               */
    float scale;            /* finite, > 0                                                               */
    float distortion;       /* marble alone: finite (the other styles store 0)                           */
} rt_noise;

typedef struct rt_prim {
    int32_t type;      /* rt_prim_type                                       */
    int32_t material;  /* index into the material table                      */
    float f[6];        /* per-type parameters, see rt_prim_type              */
    float m[12];       /* cylinder object->world, rows of a 3x4 affine       */
    float m_inv[12];   /* cylinder world->object                             */
} rt_prim;

typedef struct rt_material {
    int32_t type;     /* rt_mat_type                                         */
    int32_t texture;  /* lambertian / diffuse_light / plastic (body colour): texture index, else -1 */
    float albedo[3];  /* metal; rough_metal: F0; rough_glass: the absorption coefficient sigma */
    float fuzz;       /* metal, clamped to <= 1 (material.cuh:61); rough_metal / plastic: the roughness r in [0, 1] */
    float ir;         /* dielectric; plastic: the coat's index of refraction; rough_glass: the index */
} rt_material;

typedef struct rt_texture {
    int32_t type;  /* rt_tex_type */
    float c0[3];
    float c1[3];
} rt_texture;

/* camera.cuh:9-29 constructor arguments + the derived frame the kernel uses */
typedef struct rt_camera {
    float lookfrom[3], lookat[3], vup[3];
    float vfov;        /* degrees                                            */
    float aspect;      /* width / height                                     */
    float aperture;
    float focus_dist;
    /* derived (camera.cuh:18-28), computed in fp64 and rounded once          */
    float origin[3], lower_left[3], horizontal[3], vertical[3];
    float u[3], v[3], w[3];
    float lens_radius;
} rt_camera;

/* scene-level switches for the deltas between the reference's two renderers
 * (SURVEY.md appendix A). */
#define RT_FLAG_SKY_GRADIENT 1u /* miss colour = cmake-cpu-version/main.cpp:36-38
                                   lerp(white, (0.5,0.7,1)); else the JSON
                                   "background" constant (main.cu:63)         */
#define RT_FLAG_DEFOCUS_BLUR 2u /* camera.h:34 lens sampling on (the CUDA
                                   renderer has it commented out,
                                   camera.cuh:33-34)                          */

typedef struct rt_scene_info {
    int32_t width, height, samples_per_pixel, max_depth;
    int32_t num_prims, num_materials, num_textures;
    uint32_t flags;
    float background[3];
    float russian_roulette; /* survival probability per bounce, 0 = off (rt_scene_set_russian_roulette) */
} rt_scene_info;

typedef struct rt_scene rt_scene; /* opaque; gpu-version/parser.hpp:16-32 `struct scene` */

/* ---- scene I/O -------------------------------------------------------- */

/* parse_scene(filename), gpu-version/parser.hpp:504-573.  Same schema:
 * background[3] max_depth samples_per_pixel width height
 * camera{lookfrom lookat vup vfov aperture} object.data[] material.data[]
 * texture.data[] [output_file].  Extensions: texture type "checker"
 * {even[3], odd[3]} (texture.cuh:33-57 has the class, the parser lacks it), texture type "image" {"file": ppm} or
 * {"rows", "cols", "data": [r, g, b, ...]}, object types "triangle" {v1, v2, v3, [u1, u2, u3]} and "mesh" {"file":
 * obj, ["scale", "matrix"[9], "translate"]} (expanded into triangles when parsed), "quad" {q, u, v, ["rotate": {axis,
 * angle}], ["translate"]} and "box" {min, max, ["rotate"], ["translate"]} (expanded into six quads; both written back as the
 * quads they became, and a field neither has is an error: rt_scene_add_quad),
 * optional top-level "sky_gradient": bool, "defocus_blur": bool (both default false: gpu-version renders a
 * constant background, main.cu:63, and has the lens sample disabled, camera.cuh:33-34) and
 * "russian_roulette": number in [0, 1].
 * Unknown object/material/texture "type" is a hard error (the reference
 * silently leaves the slot uninitialised). Returns NULL on failure. */
rt_scene *rt_scene_load_json(const char *path);
rt_scene *rt_scene_parse_json(const char *text, size_t len);

/* random_scene(), cmake-cpu-version/main.cpp:125-172 (and camera :89-94):
 * checker ground + 22x22 jittered small spheres + 3 big ones, sky gradient,
 * defocus blur, 16:9.  Randomness comes from Philox keyed by `seed`, drawn in
 * the order the reference draws (choose_mat, cx, cz, then material draws). */
rt_scene *rt_scene_rtiow(uint32_t seed, int width, int height, int spp, int max_depth);

/* serialise to the JSON schema above (round-trips through rt_scene_parse_json).
 * Returns bytes needed incl. NUL; writes at most cap bytes. */
size_t rt_scene_to_json(const rt_scene *s, char *out, size_t cap);

void rt_scene_free(rt_scene *s);

/* ---- programmatic scene building: the constructor argument lists of the
 *      reference classes (the C++ wrappers in rtmi.hpp call these) -------- */
rt_scene *rt_scene_new(int width, int height, int spp, int max_depth);
int rt_scene_set_background(rt_scene *s, const float rgb[3], uint32_t flags);
/* Russian roulette, the reference's 朴素光线追踪/4_0_path_tracing.py:43-46,88 (p_RR = 0.9): before every
 * closest-hit query the path survives with probability p (one extra draw; a path that does not
 * survive returns what it has collected so far) and a survivor's throughput is divided by p, so
 * the estimate stays unbiased (the reference divides after the scatter instead, which leaves the
 * last segment uncompensated: its images are darker by the factor p).  A non-parity fast mode: it changes which draws a sample
 * consumes, so images differ from p = 0 by noise, not bit for bit.  p = 0 (default) switches it off;
 * JSON: top-level "russian_roulette": p. */
int rt_scene_set_russian_roulette(rt_scene *s, float p);
/* Light sampling (next-event estimation): every lambertian vertex and every metal vertex with fuzz >= 0.05 whose
 * continuation is traced also samples one emitter -- chosen in proportion to its power (area x mean emission luminance)
 * -- and checks its visibility with a shadow ray; the light sample and the BSDF sample are combined by multiple
 * importance sampling (power heuristic).  Sampled emitters: spheres (uniform in the cone they subtend), axis-aligned
 * rects and cylinder tubes with a rigid transform (uniform by area) whose material is a diffuse_light with a solid or
 * checker texture (rt_scene_get_lights lists them); every other emitter is still reached by the BSDF sample alone.
 * Unbiased against on = 0 at the same max_depth and russian_roulette, with far less noise in scenes lit by small emitters;
 * images differ from on = 0 by noise, not bit for bit.  A scene with light sampling on and at least one sampled emitter
 * renders through the light-sampling kernels (rt_opts.variant 0, 16, 36 or 44; rt_stats.kernel_variant reports the
 * layout | 256); other variants and rt_render_hip_count refuse it.  on = 0 (default) switches it off; JSON: top-level
 * "light_sampling": true. */
int rt_scene_set_light_sampling(rt_scene *s, int on);
int rt_scene_get_light_sampling(const rt_scene *s); /* 1, 0, or -rt_status */
/* Mesh lights: with on = 1 the list of sampled emitters (rt_scene_get_lights) also holds every triangle -- the triangles of
 * an OBJ mesh among them, one light each -- whose material is a diffuse_light with a solid or checker texture and whose area
 * and power are positive and finite (a degenerate triangle is skipped); a point on it is drawn uniformly by area, the
 * density is stated with its geometric normal, vertex normals or not.  The switch only widens that list: without light
 * sampling on it changes nothing that is rendered, and with on = 0 (default) the list, the tables and every frame are what
 * they were, an emissive triangle being reached by the BSDF sample alone.  JSON: top-level "mesh_lights": true. */
int rt_scene_set_mesh_lights(rt_scene *s, int on);
int rt_scene_get_mesh_lights(const rt_scene *s); /* 1, 0, or -rt_status */
/* Light sampling in participating media: with on = 1 a scene that has media AND light sampling with something to
 * sample renders through kernels that combine them (rt_opts.variant 0, 16, 36 or 44; rt_stats.kernel_variant reports
 * layout | 2048 | 256) instead of being refused.  A medium vertex takes a light sample where a surface vertex does -- after
 * the depth count and a survived roulette draw, the three light draws behind the roulette draw -- with the phase function as
 * its density: pdf_b = 1 / (4 pi) for the stored g = 0, rt_phase_hg_eval(g, w . w_l) otherwise (w the unit direction of
 * travel), f = albedo x pdf_b without a cosine, the power heuristic against the light's density, a point, spot or distant
 * light at weight 1.  Its continuation carries pdf_b of the direction it drew, so an emitter it reaches is weighed as behind
 * a surface vertex.  A shadow ray takes NO draw: every medium, in list order, adds sigma (b - a) |d| of its stay [a, b]
 * (rt_medium_interval over the shadow ray's own range) to an optical depth tau, and an unoccluded sample is multiplied by
 * exp(-tau) (rt_media_transmittance).  Any surface occludes, glass included.  The switch acts only together with media and
 * light sampling that has something to sample: alone it changes no table and no frame.  Refused with RT_ERR_ARG beside
 * everything media refuse: the switch (acting) with a projection other than the perspective one.  Off by default; JSON:
 * top-level "media_light_sampling": true, written only when on. */
int rt_scene_set_media_light_sampling(rt_scene *s, int on);
int rt_scene_get_media_light_sampling(const rt_scene *s); /* 1, 0, or -rt_status */
/* Nested grid: a second grid level for scenes whose geometry is clustered (a detailed mesh standing in a room).  The candidate
 * search is one uniform grid whose cell comes from the extent of all primitives; a cell that a dense mesh overfills can only
 * hand its members to the set that is tested for every query.  With on = 1 such a scene -- one whose flat tables have a cell
 * list longer than the nesting threshold (64 entries), or lost primitives through an overflowing cell -- is packed in the wide
 * format with every cell above the threshold NESTED: it gets a sub-grid of its own, sized from what it holds (at most 32 cells
 * per axis, one level), and the walk steps through the sub-cells while the ray is inside it.  Such a scene renders through
 * kernel variant 52 (rt_opts.variant 0 or 52; 16 and 24 still scan it; the other grid variants fail with RT_ERR_ARG), to the
 * same image bit for bit.  A scene with nothing to nest keeps its tables, its kernel and its bytes.  Not combined with light
 * sampling: a nested scene with light sampling on and an emitter to sample fails to render with RT_ERR_ARG.
 * on = 0 (default) switches it off; JSON: top-level "nested_grid": true. */
int rt_scene_set_nested_grid(rt_scene *s, int on);
int rt_scene_get_nested_grid(const rt_scene *s); /* 1, 0, or -rt_status */
typedef struct rt_light {
    int32_t prim;        /* index into the primitive list (-1: an analytic light or the environment) */
    int32_t shape;       /* rt_prim_type: sphere, xy / xz / yz rect, cylinder, quad or -- with mesh lights on -- triangle; or RT_LIGHT_* */
    float probability;   /* selection probability (the list sums to 1)         */
    float area;          /* surface area (the cylinder's tube; a triangle's |e1 x e2| / 2; a quad's |u x v|) */
    float emission[3];   /* emission (a checker texture: its even colour)      */
    float emission_odd[3]; /* a checker texture's odd colour (else = emission) */
} rt_light;
/* the emitters light sampling samples, in list order (whether or not it is on) -> count, or -rt_status.  An environment
 * with something to sample comes last: prim = -1, shape = RT_LIGHT_ENVIRONMENT, area = 4 pi, emission = its mean radiance. */
int rt_scene_get_lights(const rt_scene *s, rt_light *out, int cap);
#define RT_LIGHT_ENVIRONMENT 100 /* rt_light.shape of the environment (outside rt_prim_type's values) */

/* ---- analytic lights: point, spot and distant -------------------
 * An analytic light has no geometry: the camera does not see it, no BSDF ray hits it, feature passes and ray queries ignore
 * it.  It acts through the light sample of a vertex alone, so only with light sampling on (rt_scene_set_light_sampling); with
 * it off the lights are not in the tables and the scene renders the bytes of the scene without them.  Its sample carries MIS
 * weight 1 (the BSDF strategy can never produce it).  Vertices that take no light sample -- dielectric, metal below fuzz
 * 0.05, glossy below the minimum roughness -- see nothing of these lights (no highlight of a delta light on a near-mirror).
 * With psel the light's selection probability, vb the throughput and fcos(w) the material's f cos towards w, at a vertex p:
 *   point    position x, intensity I (RGB per steradian): ld = x - p, d2 = ld.ld, contribution vb fcos(ld/|ld|) I / (psel d2);
 *            d2 = 0: no sample.
 *   spot     the point light times a falloff: with the unit axis a (the direction it points), c = a.(-ld/|ld|),
 *            s = clamp((c - cos(outer)) / (cos(inner) - cos(outer)), 0, 1), falloff = s^2 (3 - 2 s).
 *   distant  unit direction t TOWARDS the light, normal irradiance E (RGB), angular radius alpha in [0, 45] degrees: the
 *            sample direction w is uniform in the cone of half-angle alpha about t (alpha = 0: w = t exactly); the cone's
 *            radiance is E / (pi sin^2 alpha), so that E is the irradiance on a surface facing the light, and the
 *            contribution is vb fcos(w) E 2 / (1 + cos alpha) / psel.  The shadow ray is 4 x the scene's bounding radius long.
 * Selection weights, beside area x mean luminance of the area emitters: 4 lum(I); 2 (1 - (cos_i + cos_o) / 2) lum(I);
 * r^2 lum(E) with r the bounding radius of the primitives.  A light whose weight is not positive and finite is left out.
 * Rules (RT_ERR_SCENE from the JSON reader, RT_ERR_ARG from the calls below): colours finite, >= 0, not all zero; directions
 * finite and non-zero (normalised in fp64); 0 <= inner <= outer, 0 < outer <= 179; 0 <= angular radius <= 45.
 * Not combined with media, moving spheres or the nested grid, which refuse as light sampling refuses them.
 * JSON: top-level "lights": [{"type": "point", "position", "intensity"}, {"type": "spot", "position", "direction" | "target",
 * "intensity", "inner_angle", "outer_angle"}, {"type": "distant", "direction", "irradiance", ["angular_radius"]}]; "lights"
 * without a "light_sampling" key switches light sampling on. */
#define RT_LIGHT_POINT 101
#define RT_LIGHT_SPOT 102
#define RT_LIGHT_DISTANT 103
typedef struct rt_analytic_light {
    int32_t type;       /* RT_LIGHT_POINT / RT_LIGHT_SPOT / RT_LIGHT_DISTANT */
    float position[3];  /* point, spot */
    float direction[3]; /* spot: where it points; distant: the direction the light TRAVELS (as given, not normalised) */
    float color[3];     /* point, spot: intensity per steradian; distant: normal irradiance */
    float angle[2];     /* degrees.  spot: inner, outer; distant: angular radius, 0 */
} rt_analytic_light;
int rt_scene_add_point_light(rt_scene *s, const float position[3], const float intensity[3]); /* -> index, or -rt_status */
int rt_scene_add_spot_light(rt_scene *s, const float position[3], const float direction[3], const float intensity[3],
                            float inner_deg, float outer_deg);
int rt_scene_add_distant_light(rt_scene *s, const float direction_of_travel[3], const float irradiance[3], float angular_radius_deg);
int rt_scene_get_analytic_lights(const rt_scene *s, rt_analytic_light *out, int cap); /* -> count, or -rt_status */
int rt_scene_clear_analytic_lights(rt_scene *s);
/* rt_scene_get_lights lists them after the area emitters and before the environment: prim = -1, shape = the type, emission =
 * emission_odd = the colour as the light record holds it (a distant light's times 2 / (1 + cos alpha)), area = the measure of
 * the selection weight: 4 pi, 2 pi (1 - (cos_i + cos_o) / 2), pi r^2. */

/* ---- environment map (image-based lighting) -------------------------------
 * rows x cols fp32 RGB texels (finite, >= 0) in lat-long layout: row 0 is the zenith (+y), rows go down to -y, columns go
 * round in azimuth.  For a unit direction d
 *     v = acos(d.y) / pi,                          row = min(int(v rows), rows - 1)
 *     u = frac((atan2(-d.z, d.x) + pi) / 2 pi + rotate_deg / 360),   col = min(int(u cols), cols - 1)
 * (the sphere's u, v of object.cuh:87-93; every step one fp32 operation, acos / atan2 the fixed sequences of the hit
 * record's texture coordinates), and the radiance is scale x texel[row][col] (nearest texel, as image textures).  With an
 * environment set a ray that misses everything returns throughput x radiance(d) in place of the background and the sky
 * gradient, with no extra random draw: a map of one colour c at scale 1 renders the bytes of background = c.
 * With light sampling on (rt_scene_set_light_sampling) the environment is one more sampled emitter: directions are drawn in
 * proportion to luminance x solid angle, piecewise constant over texels (a marginal CDF over rows and a conditional CDF per
 * row, built in fp64, stored as fp32; uniform in solid angle inside the texel; pdf = pmf(texel) / solid angle of the row's
 * texels; zero-luminance texels are never drawn).  Its selection weight is r^2 x scale x sum(luminance x solid angle), r the
 * radius of the primitives' bounding sphere.  Its shadow ray has no far end; a BSDF ray from a light-sampled vertex that
 * escapes is weighted by the power heuristic.  Scenes with an environment get the wide tables and render through kernels of
 * their own (rt_opts.variant 0, 16, 36 or 44; rt_stats.kernel_variant reports layout | 1024, | 256 with light samples); other
 * variants, rt_render_hip_count and scenes whose tables have nested cells fail with RT_ERR_ARG.
 * rows = 0 clears the environment.  RT_ERR_ARG for bad arguments, RT_ERR_SCENE for negative or non-finite texels,
 * RT_ERR_LIMIT beyond 2^25 texels.  JSON: top-level "environment": {"file": path, "scale": s, "rotate": deg} or
 * {"rows": r, "cols": c, "data": [r x c x 3 numbers], ...}. */
int rt_scene_set_environment(rt_scene *s, int rows, int cols, const float *rgb, float scale, float rotate_deg);
/* the same from a file: Radiance .hdr (RGBE: flat or new-style run-length scanlines, "-Y H +X W"), PFM ("PF", either
 * endianness), or an 8-bit PNG / PPM as an LDR map (byte / 255).  RT_ERR_IO / RT_ERR_SCENE for unreadable or malformed files. */
int rt_scene_set_environment_file(rt_scene *s, const char *path, float scale, float rotate_deg);
/* size (rows = cols = 0: none), scale, rotation and, if rgb != NULL, the rows x cols x 3 texels; any pointer may be NULL */
int rt_scene_get_environment(const rt_scene *s, int *rows, int *cols, float *scale, float *rotate_deg, float *rgb,
                             size_t cap_floats);
/* Host evaluations of the device functions (no GPU needed).  eval: radiance and sampling density (per steradian) of
 * direction dir, which is normalised in fp64 and rounded to fp32 first.  sample: the direction the sampler draws from
 * (u1, u2) in [0, 1)^2 -- u1: row, then cos(theta) within its band; u2: column, then azimuth within the texel -- with the
 * radiance and density eval gives that direction (pdf 0 when the map has nothing to sample). */
int rt_environment_eval(const rt_scene *s, const float dir[3], float rgb[3], float *pdf);
int rt_environment_sample(const rt_scene *s, float u1, float u2, float dir[3], float rgb[3], float *pdf);

/* ---- homogeneous participating media (fog, smoke) ----------------
 * Up to RT_MAX_MEDIA media per scene, a list of its own: media are not primitives (not in rt_scene_get_prims, not in the
 * grid, they occlude nothing) and leave the primitive part of the packed tables alone.  A medium is a boundary -- a sphere
 * or an axis-aligned box -- filled with a density sigma >= 0 per unit world length and an albedo in [0, 1]^3; scattering is
 * isotropic.  After every closest-hit query (ray o + t d, surface winner t_s, +inf on a miss) the media are walked in list
 * order: [a, b] = the ray's stay inside the boundary clipped to [0.001, t_s]; an empty interval, or sigma = 0, takes no random
 * draw; otherwise ONE draw u and t = a + (-ln(1 - u) / sigma) / |d|, an event if t < b.  The smallest event t (the earlier
 * medium at equal t) wins over the surface hit: a vertex that costs one unit of depth, multiplies the throughput by the albedo,
 * emits nothing, and goes on from o + t d in the direction of a uniform point of the unit sphere (the lambertian's rejection
 * loop, three draws per attempt, normalised).  Nothing is remembered between queries, so cameras and vertices inside media,
 * overlapping media (the summed-density process) and media inside glass shells need nothing more.  Russian roulette keeps
 * its draw before the query.
 * A scene with media gets the wide tables and renders through kernels of its own (rt_opts.variant 0, 16, 36 or 44;
 * rt_stats.kernel_variant reports layout | 2048) through every render entry point.  Refused with RT_ERR_ARG: media together
 * with light sampling that has something to sample (unless rt_scene_set_media_light_sampling is on), with an environment map, or with nested cells; rt_render_hip_count; any
 * other variant.  Feature passes (rt_render_hip_feature) ignore media: they record the first SURFACE hit, so the denoiser's
 * guides do not see fog.
 * Errors of the add calls: RT_ERR_ARG null pointers; RT_ERR_SCENE a negative or non-finite density, an albedo outside [0, 1],
 * a radius <= 0 or non-finite bounds, a box with min >= max on an axis; RT_ERR_LIMIT the 17th medium.
 * JSON: top-level "media": {"data": [{"type": "sphere", "center", "radius", "density", "albedo"},
 * {"type": "box", "min", "max", "density", "albedo"}]}, either with an optional "g".
 *
 * Anisotropic media: a medium has an asymmetry g in [-0.99, 0.99], 0 when it is added.  g > 0 scatters forward,
 * along the direction of travel, g < 0 backward, by the Henyey-Greenstein phase function of the angle t between the arriving
 * and the leaving direction of travel: p(cos t) = (1 - g^2) / (4 pi (1 + g^2 - 2 g cos t)^(3/2)) per steradian.  |g| < 1e-3 is
 * stored as exactly 0, and such a medium is the isotropic one above, draw for draw and bit for bit; a non-finite g or
 * |g| > 0.99 is RT_ERR_SCENE, a medium id the scene does not have RT_ERR_ARG.  A vertex in a medium with stored g != 0 takes no
 * attempt of the rejection loop but TWO draws, u1 then u2, where the attempts would have been (behind the query's free-flight
 * draws; the roulette draw keeps its place): with w = d / |d|, s = (1 - g^2) / (1 - g + 2 g u1),
 * cos t = (1 + g^2 - s^2) / (2 g) clamped to [-1, 1], sin t = sqrt(max(0, 1 - cos^2 t)), p = 2 pi u2 and (t1, t2) the frame of
 * Duff et al. about w, it goes on in the direction sin t cos p t1 + sin t sin p t2 + cos t w.  The direction is drawn with the
 * phase function's own density, so the throughput is multiplied by the albedo and nothing else; the vertex costs one unit of
 * depth and emits nothing, as the isotropic one.  The refusals are those above, whatever g is.  Setting a different stored
 * value makes the scene a new version; setting the value it holds does not.  rt_scene_clear_media clears the asymmetries too.
 * JSON writes "g" only where the stored value is not 0. */
#define RT_MAX_MEDIA 16
typedef enum rt_medium_shape { RT_MEDIUM_SPHERE = 0, RT_MEDIUM_BOX = 1 } rt_medium_shape;
typedef struct rt_medium {
    int32_t shape;   /* rt_medium_shape */
    float f[6];      /* sphere {cx, cy, cz, r}; box {min.xyz, max.xyz} */
    float density;
    float albedo[3];
} rt_medium;
int rt_scene_add_medium_sphere(rt_scene *s, const float center[3], float radius, float density, const float albedo[3]); /* -> medium id, or -rt_status */
int rt_scene_add_medium_box(rt_scene *s, const float bmin[3], const float bmax[3], float density, const float albedo[3]);
int rt_scene_get_media(const rt_scene *s, rt_medium *out, int cap); /* -> count, or -rt_status */
int rt_scene_clear_media(rt_scene *s);
/* Host evaluation of the device's interval formula (no GPU needed): the part of the ray o + t d inside the boundary, clipped to
 * [0.001, t_max].  1: non-empty (a < b), with *t_in = a and *t_out = b; 0: empty; -RT_ERR_ARG for null arguments or a shape
 * that is neither a sphere nor a box. */
int rt_medium_interval(const rt_medium *m, const float orig[3], const float dir[3], float t_max, float *t_in, float *t_out);
/* Host evaluation of a shadow ray's transmittance through the scene's media (no GPU needed): over the segment
 * o + t d, t in [0.001, t_max], every medium of positive density in list order adds x = sigma * (b - a), tau = fma(x, |d|, tau)
 * with [a, b] its rt_medium_interval and |d| = sqrt(d.d); *T = exp(-tau) in fp32, exactly 1 when no stay is non-empty.
 * A shadow ray to a light point y has d = y - o and t_max = 0.999. */
int rt_media_transmittance(const rt_scene *s, const float orig[3], const float dir[3], float t_max, float *T);
int rt_scene_set_medium_phase(rt_scene *s, int medium, float g);
int rt_scene_get_medium_phase(const rt_scene *s, int medium, float *g); /* the STORED value: 0 after a set of 5e-4 */
/* Host evaluations of the device's phase function (no GPU needed).  sample: the direction a vertex with asymmetry g (non-zero,
 * |g| <= 0.99: else RT_ERR_ARG) leaves in, from the direction of travel `dir` (any length > 0) and its two draws; unit length
 * up to rounding.  eval: p(cos t) per steradian, for any g in (-1, 1). */
int rt_phase_hg_sample(float g, const float dir[3], float u1, float u2, float out[3]);
float rt_phase_hg_eval(float g, float cos_theta);

/* ---- motion blur: linearly moving spheres over a per-sample shutter time ----------------
 * Up to RT_MAX_MOVING_SPHERES moving spheres per scene, a list of its own: they are not in rt_scene_get_prims and not in the
 * grid, and leave the primitive part of the packed tables alone.  They are surfaces: they occlude and carry any material of
 * the scene, a diffuse_light included.  At shutter time s in [0, 1) the centre is c(s) = center0 + s (center1 - center0),
 * per component fmaf(s, v, center0) with v = center1 - center0 computed once in fp32.
 * A sample of a scene with at least one mover has ONE time s for its whole path.  s is not a draw of the sample's stream: it is
 * the top 24 bits of word 0 of Philox4x32-10(counter = (pixel_id, sample_index, 1, 0), key = (seed_lo, seed_hi)) x 2^-24 -- the
 * block beside the one that seeds the stream (whose counter word 2 is 0) --, so every other draw of the sample stays where
 * it is (rt_shutter_time).
 * Every closest-hit query first finds its winner among the static primitives as before, then tests the movers in list order
 * against the sphere (c(s), radius) with sphere::hit's operation sequence (oc, a, half_b, c, discriminant, the near root, then
 * the far one; t_min = 0.001) and t_max = the nearest t so far: a mover behaves as a sphere listed behind every primitive, so
 * at equal t a mover wins over a static primitive and a later mover over an earlier one.  The hit record is p = o + t d, the
 * outward normal (p - c(s)) / radius, face-turned, and (u, v) for image textures as for a static sphere.
 * A scene with a mover gets the wide tables and renders through kernels of its own (rt_opts.variant 0, 16, 36 or 44;
 * rt_stats.kernel_variant reports layout | 4096) through every render entry point.  Refused with RT_ERR_ARG: movers together
 * with light sampling that has something to sample, with an environment map, with media or with nested cells;
 * rt_render_hip_count; feature passes (the denoiser's guides would show the scene at no particular time); any other variant.
 * Errors of the add call: RT_ERR_ARG null pointers; RT_ERR_SCENE a radius <= 0 or not finite, non-finite centres, an unknown
 * material; RT_ERR_LIMIT the 65th mover.
 * JSON: an object {"type": "moving_sphere", "center0", "center1", "radius", "material"} in "object". */
#define RT_MAX_MOVING_SPHERES 64
typedef struct rt_moving_sphere {
    float center0[3]; /* the centre at s = 0 */
    float center1[3]; /* ... and at s = 1 */
    float radius;
    int32_t material;
} rt_moving_sphere;
int rt_scene_add_moving_sphere(rt_scene *s, const float center0[3], const float center1[3], float radius, int material); /* -> mover id, or -rt_status */
int rt_scene_moving_sphere_count(const rt_scene *s); /* -> count, or -rt_status */
int rt_scene_get_moving_spheres(const rt_scene *s, rt_moving_sphere *out, int cap); /* -> count, or -rt_status */
int rt_scene_clear_moving_spheres(rt_scene *s);
/* Host evaluation of the device's intersection (no GPU needed): the mover at shutter time s against the ray orig + t dir over
 * [0.001, t_max].  1: a hit, with *t its ray parameter; 0: a miss; -RT_ERR_ARG for null arguments (t may be null). */
int rt_moving_sphere_hit(const rt_moving_sphere *m, float s, const float orig[3], const float dir[3], float t_max, float *t);
/* the shutter time of sample `sample` of pixel `pixel` (y * width + x) under `seed`, as the kernels evaluate it */
float rt_shutter_time(uint64_t seed, uint32_t pixel, uint32_t sample);
/* camera(lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist) camera.cuh:9-15;
 * aspect <= 0 -> width/height, focus_dist <= 0 -> |lookfrom-lookat| (parser.hpp:122-124) */
int rt_scene_set_camera(rt_scene *s, const float lookfrom[3], const float lookat[3],
                        const float vup[3], float vfov, float aspect, float aperture,
                        float focus_dist);
/* Camera projections: how (s, t) in [0, 1]^2 -- s to the right, t upwards -- becomes a ray.  u, v, w are the frame
 * of rt_camera, f = -w the forward direction, a the aspect ratio, fd the focus distance.  Every projection defines a pinhole
 * ray (o, D) with |D| = fd; with RT_FLAG_DEFOCUS_BLUR the ray of the lens sample (lx, ly) is (o + off, D - off), off =
 * lens_radius (lx u + ly v), so every lens ray of a sample passes through o + D, as the perspective camera's do.
 *   RT_PROJ_PERSPECTIVE   the default: rt_scene_set_camera's pinhole / thin lens.  No parameters.
 *   RT_PROJ_ORTHOGRAPHIC  params[0] = height h > 0 in world units: o = lookfrom + (s - 1/2) h a u + (t - 1/2) h v, D = fd f.  The
 *                         camera's vfov is ignored.
 *   RT_PROJ_PANORAMIC     params = {hfov in (0, 360], vfov in (0, 180]} degrees (null: 360, 180), a lat-long frame: phi = (s - 1/2)
 *                         hfov, psi = (t - 1/2) vfov, D = fd (cos psi (cos phi f + sin phi u) + sin psi v), o = lookfrom.  Increasing
 *                         s turns right, so the frame reads correctly from inside -- mirrored against the column order of an
 *                         environment map (rt_scene_set_environment).
 *   RT_PROJ_FISHEYE       params[0] = fov in (0, 360] degrees (null: 180), equidistant: (px, py) = ((2s - 1) max(a, 1), (2t - 1)
 *                         max(1 / a, 1)), r = |(px, py)|, theta = r fov / 2, D = fd (cos theta f + (sin theta / r)(px u + py v)),
 *                         o = lookfrom: the image circle is inscribed in the frame's shorter side.  A sample with r > 1 has no
 *                         path: it takes its draws, adds zero radiance (zeros in a feature pass) and counts as a sample.
 * The projection survives rt_scene_set_camera and rt_scene_override; a non-finite or out-of-range parameter or an unknown type
 * is RT_ERR_ARG and changes nothing.  A scene with a projection other than the perspective one renders through kernel
 * instances of its own (csrc/camera_kernel.h) over the general layouts.  Refused at render time (RT_ERR_ARG): the compact
 * sphere-only layouts (variants 2 and 6: use 0, 16, 36 or 44); rt_render_hip_count; a scene that also has a material with an
 * alpha mask (those kernels are not built: remove the masks or render in perspective). */
typedef enum rt_projection_type {
    RT_PROJ_PERSPECTIVE = 0, RT_PROJ_ORTHOGRAPHIC = 1, RT_PROJ_PANORAMIC = 2, RT_PROJ_FISHEYE = 3
} rt_projection_type;
int rt_scene_set_projection(rt_scene *s, int type, const float params[2]);
int rt_scene_get_projection(const rt_scene *s, int *type, float params[2]); /* unused parameters read 0 */
int rt_scene_add_solid_color(rt_scene *s, const float rgb[3]);                 /* -> texture id */
int rt_scene_add_checker(rt_scene *s, const float even[3], const float odd[3]); /* -> texture id */
int rt_scene_add_lambertian(rt_scene *s, int texture);                         /* -> material id */
int rt_scene_add_metal(rt_scene *s, const float albedo[3], float fuzz);
int rt_scene_add_dielectric(rt_scene *s, float ir);
/* Glossy materials: a GGX lobe with height-correlated Smith masking, sampled through its visible normals.
 * rough_metal: Schlick Fresnel about F0 = albedo (each component finite and in [0, 1]).  plastic: a diffuse body of the
 * texture's colour (solid, checker or image) under a clear coat of index ior (finite, > 1).  roughness is finite and in [0, 1]
 * (alpha = max(roughness^2, 1e-3)); with light sampling on, a vertex of either takes a light sample iff roughness >= 0.05.
 * Anything else is RT_ERR_ARG.  A scene with either runs the general (triangle / texture) kernels.  -> material id or -rt_status */
int rt_scene_add_rough_metal(rt_scene *s, const float albedo[3], float roughness);
int rt_scene_add_plastic(rt_scene *s, int texture, float ior, float roughness);
/* Rough glass (the model: csrc/rt_glass.h): reflection or refraction about a microfacet normal of the same GGX
 * lobe, tinted by the distance travelled inside the object.  ir finite and > 1, roughness finite and in [0, 1], absorption
 * (NULL: clear) three finite coefficients >= 0 per unit world length; anything else is RT_ERR_ARG.
 * At a vertex with face-turned shading normal n, in the frame of Duff et al. about n, wo = -unit(d), alpha =
 * max(roughness^2, 1e-3), eta = front ? 1 / ir : ir:
 *   wo.z <= 0: absorbed, no draws, no light sample.  Otherwise three draws uf, u1, u2; h = the visible normal of the lobe from
 *   (u1, u2), c = wo.h; s2 = eta^2 (1 - c^2); F = 1 if s2 >= 1, else with ct = sqrt(1 - s2), rs = (eta c - ct) / (eta c + ct),
 *   rp = (c - eta ct) / (c + eta ct): F = (rs^2 + rp^2) / 2 (the exact unpolarised Fresnel term).
 *   uf < F: wi = 2 c h - wo, absorbed if wi.z <= 0, pdf_b = F G1(wo) D(h) / (4 wo.z).
 *   else:   wi = (eta c - ct) h - eta wo, absorbed if wi.z >= 0; an emitter the continuation reaches counts at full weight.
 *   Attenuation, both: Tr G2(wo, wi) / G1(wo), Lambda(wi) of wi as it stands.  No eta^2 radiance scaling (as dielectric).
 *   Tr = 1 on a front hit, exp(-sigma t |d|) per channel on a back hit (t |d|: the length of the segment that arrived).
 *   The rule is stateless: right for solid closed objects, for a camera inside one and for objects embedded in the glass seen
 *   from the embedded object; a segment that ENDS on another material inside the glass is not tinted, and air bubbles are not
 *   handled (both out of scope, with nested or overlapping glass).
 * With light sampling on, a vertex takes a light sample iff roughness >= 0.05 and wo.z > 0; the light strategy covers the
 * reflection hemisphere alone: for wl.z > 0, h_l = unit(wo + wl): f cos = Tr F(wo.h_l) D(h_l) G2 / (4 wo.z), pdf_b =
 * F(wo.h_l) G1(wo) D(h_l) / (4 wo.z); zero for wl.z <= 0 (no light sample through the surface).  The feature passes report
 * albedo 1 and the shading normal.  A scene with one runs the general (triangle / texture) kernels.  -> material id or -rt_status */
int rt_scene_add_rough_glass(rt_scene *s, float ir, float roughness, const float absorption[3]);
/* The metallic-roughness material (the model: csrc/rt_pbr.h), glTF 2.0's: a base colour texture of any type, a
 * metallic factor mf and a roughness factor rf, finite and in [0, 1], a coat index ior, finite and > 1, and optionally one
 * metallic-roughness map, a texture of any type whose G channel scales the roughness and whose B channel scales the metalness
 * (an ORM image drops in unchanged).  The base texture must exist; the map must be an existing texture or -1 (none), on a pbr
 * material only; anything else is RT_ERR_ARG.
 * Per-hit parameters are 8-bit by definition: with the base colour c, the map's channels G, B at the hit (1 without a map),
 *   byte(x) = (uint)fma(clamp(x, 0, 1), 255, 0.5) in fp32:  c8 = byte(c) per channel, r8 = byte(rf G), m8 = byte(mf B),
 *   and the values are c8 / 255, r = r8 / 255, m = m8 / 255 (one fp32 division each): an image's texel is used exactly, solid,
 *   checker and noise sources are rounded to that grid.
 * A vertex seen from above its shading normal takes three draws ul, u1, u2, in plastic's order, whatever its metalness:
 *   ul < m:  the vertex is a rough_metal with F0 = c8 / 255 and roughness r (ul is otherwise unused);
 *   else:    a plastic with body c8 / 255, the coat's r0 from ior, roughness r, and lobe draw ul' = (ul - m) / (1 - m);
 *   alpha = max(r r, 1e-3) in fp32.  Everything after that is the chosen material's rule, for the scatter step and -- iff
 *   r >= 0.05 and the vertex is not below the surface -- for the light sample: both see the same, already chosen, BSDF.  The
 *   expectation over the choice is m metal(c) + (1 - m) dielectric(c).
 * The albedo feature pass reports c8 / 255; a bump applies as on the other glossy materials.  A scene with one runs the general
 * (triangle / texture) kernels.  The map lives beside the material table, as the bumps do: rt_material is unchanged.
 * rt_scene_add_pbr -> material id or -rt_status; the other two -> rt_status (get: *texture = the map's texture id, -1: none) */
int rt_scene_add_pbr(rt_scene *s, int base_texture, float metallic, float roughness, float ior);
int rt_scene_set_pbr_map(rt_scene *s, int material, int texture);
int rt_scene_get_pbr_map(const rt_scene *s, int material, int *texture);
int rt_scene_add_diffuse_light(rt_scene *s, int texture);
int rt_scene_add_sphere(rt_scene *s, const float center[3], float radius, int material); /* -> prim id */
/* axis: 0 = xy_rect (a=x,b=y,k=z), 1 = xz_rect, 2 = yz_rect */
int rt_scene_add_rect(rt_scene *s, int axis, float a0, float a1, float b0, float b1, float k,
                      int material);
/* cylinder(radius, zmin, zmax, mat) then rotate(axis, degrees) then translate(offset),
 * composed as parser.hpp:423-440 does (o2w = T * R); pass NULL to skip either. */
int rt_scene_add_cylinder(rt_scene *s, float radius, float zmin, float zmax, int material,
                          const float rot_axis[3], float rot_degrees, const float translate[3]);
/* negative ids above = -rt_status */

/* Image texture, taichi-version/material.py:96-110, 137-144 (the reference keeps one 100 x 100 image): `rgb` holds
 * rows x cols texels, 3 bytes each (R, G, B), row-major.  value(u, v, p) = texel[int(frac(u) * rows)][int(frac(v) *
 * cols)] / 255 (frac(x) = x - floor(x); an index that rounds up to rows / cols is clamped).  -> texture id.
 * The hit record's u, v (sphere object.cuh:87-93, rects :113-114, cylinder :283-288, triangle hittable.py:233)
 * are only evaluated for hits on materials with an image texture. */
int rt_scene_add_image_texture(rt_scene *s, int rows, int cols, const uint8_t *rgb);
/* the same from a file: PNG (8 bits per channel, non-interlaced; grey, grey + alpha, RGB, RGBA or palette; alpha is
 * kept as a plane of its own for grey + alpha, RGBA and a palette with a tRNS chunk -- DESIGN 7v, below) or binary / text PPM (P6 / P3, maxval 255).  The reference reads its assets through OpenCV, and two of its
 * three "*.png" textures are JPEG files: convert those once
 * (`python -c "from PIL import Image; Image.open('bricks2.png').convert('RGB').save('bricks2.ppm')"`). */
int rt_scene_add_image_texture_file(rt_scene *s, const char *path);
/* rows / cols of image texture `texture` and, if out != NULL, its rows*cols*3 bytes; -rt_status on error */
int rt_scene_get_image(const rt_scene *s, int texture, int *rows, int *cols, uint8_t *out, size_t cap);
/* Alpha cutouts.  An image texture may carry an alpha plane: rows*cols*4 bytes R G B A here, or a file with alpha.
 * Colour lookups ignore the plane; it only serves as a material's alpha mask (rt_scene_set_alpha). -> texture id */
int rt_scene_add_image_texture_rgba(rt_scene *s, int rows, int cols, const uint8_t *rgba);
/* rows / cols of image texture `texture` and, if out != NULL and the image has an alpha plane, its rows*cols alpha bytes.
 * -> 1: the image has a plane, 0: it has none (every texel counts as 255; out is left alone); -rt_status on error */
int rt_scene_get_image_alpha(const rt_scene *s, int texture, int *rows, int *cols, uint8_t *out, size_t cap);
/* The alpha mask of `material`: the alpha byte a8 of image texture `texture` at the hit record's (u, v) -- the nearest texel,
 * as an image-textured material reads its colour: the row from u, the column from v, clamped to the last row and column --
 * against the cutoff byte c8 = clamp(ceil(255 x cutoff), 1, 255), computed once in fp64 (0.5 -> 128).  The hit is TRANSPARENT
 * iff a8 < c8, a comparison of integers.  A transparent hit is no vertex: nothing of its material is evaluated (no texture,
 * bump or normal map, no Beer-Lambert segment, no emission), it takes no random draw, counts no bounce and plays no Russian
 * roulette; the ray goes on from the hit point p = o + t d in the same direction with the usual t_min, so a surface closer
 * than t_min behind a hole is skipped as behind any vertex (two coincident cards do not show through each other's holes).
 * A shadow ray's far end stays where it was.  This happens inside one closest-hit query: for camera and BSDF rays, for the
 * shadow rays of light sampling (area, mesh, analytic and environment lights) and for the first-hit feature passes, whose
 * albedo, normal and depth are those of the first OPAQUE hit, the depth measured from the camera.  One query passes through
 * at most 64 transparent hits; the 65th masked hit of the query counts as opaque whatever its texel says.  The texture may
 * be the material's own base-colour image (the usual RGBA leaf).  On every material but diffuse_light and on every primitive
 * type.  RT_ERR_ARG for an unknown material, a diffuse_light, a texture that is not an image or has no alpha plane, a cutoff
 * outside (0, 1] or not finite.  texture = -1 removes the mask.  Refused with RT_ERR_ARG when rendered: a moving sphere whose
 * material carries a mask; a scene with both a medium and a masked material; the compact sphere-only kernel layouts
 * (variants 2 and 6); rt_render_hip_count (the counting kernels carry no masks).  The ray queries (rt_trace_hip) stay geometric: they return the closest hit whatever its mask says;
 * the record carries the material and (u, v), so a caller can look the mask up.  rt_material is unchanged. */
int rt_scene_set_alpha(rt_scene *s, int material, int texture, float cutoff);
/* the alpha mask of `material` (either pointer may be NULL): texture -1 and cutoff 0 where it has none; RT_ERR_ARG: no such material */
int rt_scene_get_alpha(const rt_scene *s, int material, int *texture, float *cutoff);
/* Noise texture: value(p) = c0 + s (c1 - c0) per channel with s from `noise` at the world-space hit point (on
 * a moving sphere too: the texture swims, as the checker does).  Usable wherever a texture id is: lambertian, plastic (body
 * colour) and diffuse_light; such an emitter emits what the texture says at the hit and, like an image-textured one, is not
 * among the sampled lights.  Colours are finite and >= 0 (they may exceed 1), scale finite and > 0, octaves in 1..8, style
 * in 0..2; for marble, axis in 0..2 and distortion finite (the other styles have neither: what the caller's record holds
 * there is not read, and zeros are stored).  Anything else is RT_ERR_ARG.  A scene with one runs the general (triangle /
 * texture) kernels.  -> texture id or -rt_status */
int rt_scene_add_noise_texture(rt_scene *s, const float c0[3], const float c1[3], const rt_noise *noise);
/* the parameters of noise texture `texture`; RT_ERR_ARG if it is none */
int rt_scene_get_noise(const rt_scene *s, int texture, rt_noise *out);
/* Bump mapping: the scalar s(p) of noise texture `texture` as a height field on material `material`.  At a
 * surface vertex with face-turned shading normal n, face-turned geometric normal g, ray direction d and sigma = +1 on a front
 * hit, -1 on a back hit (height is measured along the OUTWARD normal): G = grad s(p) (analytic), Gt = G - (G . n) n,
 * b = n - sigma strength Gt, n' = b / |b|; n' replaces n where it is finite, n' . g > 0 and n' . d < 0.  Only the height is
 * used, not the texture's colours.  The hit point, front, t, (u, v), emitter hits and the ray queries stay geometric.  On
 * lambertian, metal, dielectric, rough_metal, plastic, rough_glass and pbr; RT_ERR_ARG for an unknown material, a diffuse_light, a texture that
 * is not an RT_TEX_NOISE or a strength that is not finite.  texture = -1 or strength = 0 removes the bump.  A scene with one
 * runs the general (triangle / texture) kernels; a moving sphere whose material carries one is refused when rendered.
 * The bumps live beside the material table: rt_material is unchanged.  (RT_ERR_ARG too for a material that carries a normal
 * map, below: a material takes one of the two.) */
int rt_scene_set_bump(rt_scene *s, int material, int texture, float strength);
/* the bump of `material` (either pointer may be NULL): texture -1 and strength 0 where it has none; RT_ERR_ARG: no such material */
int rt_scene_get_bump(const rt_scene *s, int material, int *texture, float *strength);
/* Tangent-space normal maps: the texel of image texture `texture` at the hit record's (u, v) (the nearest texel, as
 * an image-textured material reads its colour) as a direction in the surface's tangent frame, on material `material`.
 * Decoding: x = max((r8 - 128) / 127, -1), y from g8, z from b8 (byte 128 is 0, byte 255 is 1); a texel with r8 == g8 == 128 or
 * z <= 0 leaves the normal alone.  R runs along +dp/du, G along +dp/dv of the primitive's own (u, v), B along the outward
 * normal.  With n the face-turned shading normal, g the face-turned geometric one, d the ray's direction, sigma = +1 on a front
 * hit, -1 on a back hit, T and B the primitive's dp/du and dp/dv:  T' = unit(T - (T.n) n),  B' = unit(B - (B.n) n - (B.T') T')
 * (zero or not finite: cross(sigma n, T')),  b = sigma scale (x T' + y B') + z n,  n' = b / |b|;  n' replaces n where it is
 * finite, n'.g > 0 and n'.d < 0; T' zero or not finite (a sphere's pole, a triangle without usable uv): n stays.  The hit
 * point, front, t, (u, v), emitter hits and the ray queries stay geometric.  On every material but diffuse_light; RT_ERR_ARG for
 * an unknown material, a diffuse_light, a texture that is not an RT_TEX_IMAGE, a scale that is not finite, or a material that
 * carries a bump (and rt_scene_set_bump refuses a material that carries a map).  texture = -1 or scale = 0 removes the map.
 * A moving sphere whose material carries one is refused when rendered.  The maps live beside the material table:
 * rt_material is unchanged. */
int rt_scene_set_normal_map(rt_scene *s, int material, int texture, float scale);
/* the normal map of `material` (either pointer may be NULL): texture -1 and scale 0 where it has none; RT_ERR_ARG: no such material */
int rt_scene_get_normal_map(const rt_scene *s, int material, int *texture, float *scale);
/* Quads and boxes.  quad(Q, u, v, material): the parallelogram Q, Q + u, Q + u + v, Q + v, whose normal is along
 * u x v; then rotate(axis, degrees) then translate(offset), the cylinder's pair and order (pass NULL to skip either).  The
 * transform is applied to Q, u, v here, in fp64, and rounded once: what is stored, rendered and written to JSON is the quad it
 * became.  A quad whose material is a diffuse_light with a solid or checker texture is one of the sampled emitters
 * (rt_scene_get_lights), uniform by area.  RT_ERR_SCENE: |u x v|^2 not positive or not finite, a value not finite, a rotation
 * axis of zero length.  A scene with a quad runs the general (triangle / texture) kernels.  -> prim id or -rt_status */
int rt_scene_add_quad(rt_scene *s, const float q[3], const float u[3], const float v[3], int material,
                      const float rot_axis[3], float rot_degrees, const float translate[3]);
/* box(min, max, material): six quads over [min, max] (min < max on every axis) in the order +z, -z, +x, -x, +y, -y, every
 * u x v pointing outward -- so `front` is the outside and a dielectric box is a solid block of glass -- with the same optional
 * transform about the origin.  All six are added or none.  -> the prim id of the first of the six, or -rt_status */
int rt_scene_add_box(rt_scene *s, const float min[3], const float max[3], int material, const float rot_axis[3],
                     float rot_degrees, const float translate[3]);
/* Triangle(v1, v2, v3, u1, u2, u3, material), taichi-version/hittable.py:95-110; uv pointers may be NULL (zeros) */
int rt_scene_add_triangle(rt_scene *s, const float v1[3], const float v2[3], const float v3[3],
                          const float uv1[2], const float uv2[2], const float uv3[2], int material);
/* readobj + the placement loop of taichi-version/main.py:23-41, 110-118: "v x y z", "vt u v", "f a b c" lines (1-based;
 * a face corner "a", "a/t" or "a/t/n"; without t the texture coordinate of corner a is vt[a], as in the reference);
 * every vertex is mapped to scale * (M v) + translate (M = 3x3 row-major, NULL = identity).  -> triangles added */
int rt_scene_add_obj(rt_scene *s, const char *path, int material, float scale, const float matrix[9],
                     const float translate[3]);

/* Smooth shading: a triangle with three vertex normals.  Geometry, t, the point, (u, v), `front` and the
 * tie rule are the flat triangle's; where a material scatters (and in the normal feature buffer and rt_hit.normal)
 * the normal is s = a1 n1 + a2 n2 + a3 n3, a_i the area of the sub-triangle opposite corner i over the whole (the three
 * area weights of (u, v), each with the corner at which it is 1), normalised and turned into the hemisphere of the
 * face-turned geometric normal; s zero or not finite: the geometric normal.  An emitter hit keeps the
 * geometric normal.  n1, n2, n3 are normalised in fp64 and rounded once; a NULL, non-finite or zero-length normal
 * is RT_ERR_ARG.  -> prim id */
int rt_scene_add_triangle_normals(rt_scene *s, const float v1[3], const float v2[3], const float v3[3],
                                  const float n1[3], const float n2[3], const float n3[3],
                                  const float uv1[2], const float uv2[2], const float uv3[2], int material);
/* where the vertex normals of a mesh come from */
typedef enum rt_mesh_normals {
    RT_MESH_NORMALS_FLAT = 0,   /* none: rt_scene_add_obj                                                          */
    RT_MESH_NORMALS_FILE = 1,   /* the file's "vn x y z" lines through the corners "a//n" and "a/t/n" (1-based; an n
                                   out of range is an error), mapped by the inverse transpose of scale * M and
                                   renormalised; a corner without n takes its face's normal                         */
    RT_MESH_NORMALS_SMOOTH = 2  /* generated: per corner the normalised angle-weighted sum of the face normals of
                                   the triangles that meet at the corner's (placed) vertex position and whose face
                                   normal lies within crease_degrees of the corner's own face                        */
} rt_mesh_normals;
/* rt_scene_add_obj with vertex normals; crease_degrees (0..180) is read by RT_MESH_NORMALS_SMOOTH alone.
 * -> triangles added */
int rt_scene_add_obj_normals(rt_scene *s, const char *path, int material, float scale, const float matrix[9],
                             const float translate[3], int mode, float crease_degrees);
/* every "mesh" of the scene files loaded from here on (this thread) takes its normals this way instead of its own
 * "normals" / "crease_angle" (the CLI's --mesh-normals); mode < 0: back to what the files say */
void rt_set_mesh_normals_override(int mode, float crease_degrees);

/* ---- animation (gpu-version/blue.py, blue2.py, dna.py: the frame harness) ----- */
/* blue.py:16-19 / blue2.py:16-19: add `degrees` to rotate.angle of every cylinder that has a
 * "rotate" and rebuild its transform; returns the number of cylinders changed (or -rt_status). */
int rt_scene_rotate_cylinders(rt_scene *s, double degrees);
int rt_scene_set_output_file(rt_scene *s, const char *path);
/* dna.py:17-98: the DNA frame at `angle_degrees` -- 60 emissive spheres + 30 emissive rotated
 * cylinders (3 helices x 10 rungs) placed into a copy of `base` (camera, background, size: the
 * reference uses basic_scene.json); base == NULL uses that file's values. */
rt_scene *rt_scene_dna(const rt_scene *base, double angle_degrees);
rt_scene *rt_scene_clone(const rt_scene *s);

/* CLI overrides -w -h -spp -d (cmake-cpu-version/main.cpp:71-81); <= 0 keeps the
 * value. Re-derives the camera when the aspect changes. */
int rt_scene_override(rt_scene *s, int width, int height, int spp, int max_depth);

/* ---- table read-back (host logic tests, checker input) ----------------- */
int rt_scene_get_info(const rt_scene *s, rt_scene_info *out);
int rt_scene_get_camera(const rt_scene *s, rt_camera *out);
int rt_scene_get_prims(const rt_scene *s, rt_prim *out, int cap);         /* -> count */
int rt_scene_get_materials(const rt_scene *s, rt_material *out, int cap); /* -> count */
int rt_scene_get_textures(const rt_scene *s, rt_texture *out, int cap);   /* -> count */

/* The device tables the host builds for a scene (no GPU needed: host logic tests, tools).  The reference rebuilds its object
 * graph on the device (move_to_device<<<1,1>>>, main.cu:374-446); here the host flattens the scene into ONE image of 16-byte
 * records -- sphere slots, the other primitives' records and boxes, the uniform grid over every primitive type (cells + lists),
 * cold records, materials -- which one memcpy uploads (csrc/device_scene.h, csrc/pack.hip pack_scene).  (The parameters of
 * the noise textures, DESIGN 7o, are one record each behind the image textures' texels: {scale, distortion, seed, style |
 * axis << 2 | octaves << 4}; a material with such a texture holds the record's offset in the fourth word of its second
 * record.  No field here says where they begin: a scene without a noise texture has none and packs to the bytes it did.
 * The bumps, DESIGN 7p, follow them the same way: one record per bumped material, {offset of the height texture's noise
 * record, strength, 0, 0}, whose offset the material holds in the fourth word of its third record; none without a bump.
 * The normal maps, DESIGN 7u, follow the bumps: one record per mapped material, {word offset of the map's texels, rows, cols,
 * scale}; the material holds MINUS its offset in that same word; none without a map.
 * The alpha masks, DESIGN 7v: when any material carries a mask, one record per material straight behind the material table,
 * {word offset of the mask's texels, rows, cols, c8}, rows 0 where the material has none; a texel word's top byte then holds
 * 255 - a8.
 * The pbr materials' side records, DESIGN 7t, follow those: three records per pbr material, in material order -- {metallic
 * factor, roughness factor, 0, 0}, then the map's texture as a material's second and third record hold theirs (no map: solid
 * white) -- whose offset the material holds in the second word of its first record; none without a pbr material.) */
typedef struct rt_table_info {
    int32_t image_floats;      /* size of the image (rt_scene_table_image) */
    int32_t grid_wide;         /* 1: wide tables (32-bit entries, two words per cell: every primitive type listed); 0: compact
                                  (sphere-only scenes whose tables fit LDS: 16-bit entries, one word per cell); 2: wide tables
                                  with nested cells (rt_scene_nested_info; grid_cells counts the top level's) */
    int32_t grid_sheet;        /* compact tables, grid one cell high */
    int32_t grid_cells, grid_n[3];
    float grid_min[3], grid_size[3];
    float ob_near2, ob_far2;   /* squared reach of the lists' near / far tier (|ray origin|^2) */
    int32_t ns, np, ncl;       /* sphere slots, leading always-tested slots, clusters of 8 (+ 1 never-hit slot each) behind them */
    int32_t nr, nc, nt;        /* rectangles, cylinders, triangles ... (quads, DESIGN 7q, are not counted here: their hot and
                                  cold records follow the triangles' with the triangles' strides, grouped ids from
                                  ns + nr + nc + nt on, in list order behind the always-tested ones) */
    int32_t nr_a, nc_a, nt_a;  /* ... of which the leading ones are tested for every query instead of being listed */
    int32_t off_grid_cells, off_grid_items;                         /* record (float4) offsets into the image */
    int32_t off_sph_cold, off_rect_cold, off_cyl_cold, off_tri_cold; /* cold records: {.., material, list index, kind} */
    int32_t off_rect_hot, off_cyl_hot, off_tri_hot;
    int32_t hot_bytes_grid;    /* what a grid-walk kernel stages into LDS */
    int32_t kernel_variant;    /* what rt_opts.variant = 0 renders this scene with (2, 6, 16, 36, 44 or 52; | 256 light sampling,
                                  | 1024 an environment map, | 2048 participating media, | 4096 moving spheres) */
} rt_table_info;
int rt_scene_table_info(const rt_scene *s, rt_table_info *out);
/* The nested cells of the scene's tables (rt_scene_set_nested_grid); all zero while the tables are flat.  A nested cell's header
 * in the cell table is {index of its sub-grid, 1023} (n_near = 1023 with n_all = 0: no plain cell has n_near > n_all).  Sub-grid
 * i is the four records at off_sub_grids + 4 i: {min.xyz, first cell (bits)} {1 / size.xyz, 0} {size.xyz, 0} {nx, ny, nz (bits), 0};
 * its cells are the nx ny nz headers from `first cell` on in the cell table (same numbering as the top level: they follow its
 * grid_cells headers, from first_sub_cell), in the wide format, and their lists lie in the item table. */
typedef struct rt_nested_info {
    int32_t cells;           /* nested cells (= sub-grids) */
    int32_t sub_cells;       /* cells of all sub-grids */
    int64_t sub_items;       /* list entries of all sub-cells */
    int32_t off_sub_grids;   /* record (float4) offset of the sub-grid records */
    int32_t off_sub_cells;   /* record offset of the first sub-cell header (two headers per record) */
    int32_t first_sub_cell;  /* ... and its index in the cell table */
    int32_t threshold;       /* a cell with more list entries (near + far spheres + others) was nested */
    int32_t axis_cap;        /* most cells per axis of a sub-grid */
    int32_t longest;         /* longest list of a cell a walk can meet (plain cells and sub-cells) */
} rt_nested_info;
int rt_scene_nested_info(const rt_scene *s, rt_nested_info *out);
/* The quads of the scene's tables, which rt_table_info does not count: *nq of them, of which the leading *nq_a are
 * tested for every query instead of being listed.  Quad k has the grouped id ns + nr + nc + nt + k, its hot records at
 * off_tri_hot + 5 (nt + k) and its cold records at off_tri_cold + 2 (nt + k), word 1 of the first: its list index. */
int rt_scene_quad_counts(const rt_scene *s, int32_t *nq, int32_t *nq_a);
/* copies min(cap_floats, image_floats) floats of the image; returns image_floats, or -rt_status */
int rt_scene_table_image(const rt_scene *s, float *out, int cap_floats);

/* ---- render ------------------------------------------------------------ */

typedef struct rt_opts {
    uint64_t seed;       /* Philox key that seeds every (pixel, sample) stream; the
                            reference seeds curand with the pixel id (main.cu:120-125) */
    int32_t device;      /* HIP device ordinal                                 */
    /* row-tile shard (multi-GPU): this call renders the row tiles
     *   t = tile_first, tile_first + tile_stride, ...   (< ceil(H / tile_rows))
     * tile t covers image rows [t*tile_rows, min(H,(t+1)*tile_rows)).
     * tile_stride <= 1 and tile_first == 0 -> whole image.                   */
    int32_t tile_rows;   /* 0 -> 8                                             */
    int32_t tile_first;
    int32_t tile_stride;
    /* How the tiles are dealt out to the tile_stride shards (N = tile_stride).  0: the plain interleave above.
     * 1: ROTATED interleave -- of every group of N consecutive tiles the shard tile_first owns one, and which one rotates
     *    from group to group: its k-th tile is k N + ((tile_first - k) mod N), i.e. tile t belongs to shard (t + t / N) mod N:
     *    no shard keeps one row phase of the image for itself.
     * 2: THERE AND BACK -- groups of 2 N tiles go to shards 0 .. N-1, then N-1 .. 0: the shard's tiles are 2 N j + tile_first and
     *    2 N j + 2 N - 1 - tile_first, which cancels the trend of the cost along the image inside every group.
     * All three give every shard the same number of tiles (+-1).  rt_shard_deal() says which one rt_render_hip_tiles and
     * bench.py use for a frame: 1 when the frame has >= 4 N^2 tiles (the rotation has gone round four times), else 2
     * (RTIOW 1080p, 135 tiles, busiest shard above the mean: N = 4: 0.36 % / 0.86 %, N = 8: 2.17 % / 0.92 % for 1 / 2). */
    int32_t tile_rotate;
    /* samples per work item (one wave renders an 8x8 tile x spp_chunk samples at a time).
     * Scheduling only: the per-pixel sum is exact (64-bit fixed point, 2^-24), so the
     * framebuffer does not depend on it.  0 -> 256 (less for small frames).          */
    int32_t spp_chunk;
    int32_t sample_first; /* render samples [sample_first, sample_first+count) */
    int32_t sample_count; /* 0 -> scene spp                                    */
    uint32_t variant;     /* 0 = the product kernel for this scene, one of
                               2  uniform-grid walk, compact tables in LDS, grid one cell high (walk along x and z: RTIOW)
                               6  uniform-grid walk, compact tables in LDS (sphere-only scenes that fit LDS)
                              36  uniform-grid walk over the wide tables in LDS: every primitive type is listed in the cells
                              44  the same with the tables in global memory (scenes too large for LDS: no size limit)
                              16  no culling: the reference's linear hittable_list scan (a handful of primitives of several
                                  types; also the definition the other kernels' images are held to)
                              52  the walk of 44 over tables with nested cells (rt_scene_set_nested_grid)
                             (rt_stats.kernel_variant reports the choice).  Libraries built with RTMI_ABLATIONS (the default
                             build: rt_has_ablations()) also carry measurement variants with the same image, bit for bit:
                               1 = 6 with strict one-lane-per-pixel ownership, 40 = 6 with its tables in global memory,
                              17 = 16 with strict ownership, 24 = 16 with the tables in global memory, 32 = wave-level
                              cluster votes, 64 = per-lane cluster lists through a two-level box hierarchy, 128 = per-lane
                              cluster lists through range tables */
} rt_opts;
/* The beam table of the frame: one record of 16 uint16 words per 8x8 tile of the WHOLE frame, row-major
 * (tile (tx, ty) at ty * ceil(width / 8) + tx), whatever shard a launch renders: {count, id, id, ...}, the slots of the
 * image's sphere table that a camera ray of the tile -- any pixel of it, any jitter, any lens point -- can be flagged for by
 * the kernels' sphere test, ascending; count 0xffff: more than rt_scene_tile_beams_capacity() of them (the overflow mark: the
 * kernels run the full query there).  Variants 2 and 6 start their paths from these lists.  rt_scene_tile_beams computes the
 * table on the host (no device is touched); rt_scene_tile_beams_device builds it on device o->device (0 for a null o) as a
 * launch does and reads it back; the two agree word for word.  Both copy min(cap_tiles, tiles) records and return the number
 * of tiles, or -rt_status: RT_ERR_LIMIT for a scene without such lists (wide tables, a projection other than the perspective
 * one, a frame under 2 x 2 pixels). */
int rt_scene_tile_beams(const rt_scene *s, uint16_t *out, int cap_tiles);
int rt_scene_tile_beams_device(const rt_scene *s, const rt_opts *o, uint16_t *out, int cap_tiles);
int rt_scene_tile_beams_capacity(void);

typedef struct rt_stats {
    double kernel_ms;     /* hipEvent time of the render launches of this call */
    double upload_ms;     /* scene table upload                                */
    int32_t launches;
    int32_t local_rows;   /* rows rendered by this shard                       */
    /* exact event counts, filled only by rt_render_hip_count */
    uint64_t samples, queries, prim_tests, hits, misses;
    uint64_t scatter[4];  /* per rt_mat_type */
    uint64_t rng_draws;
    uint64_t cand_lanes, cand_waves; /* sphere candidates that reached the sqrt block: lanes / wave entries */
    uint64_t clusters_visited;       /* culling: rounds of the per-lane cluster walk, per wave (= clusters a wave tested
                                        when it votes as a whole); grid: sphere-test passes per wave */
    uint64_t wave_queries;           /* closest-hit queries executed, counted per WAVE */
    uint64_t groups_visited;         /* culling: outer boxes that passed, per wave; range tables: rounds of the per-lane
                                        candidate box tests, per wave; grid: cell-step passes per wave */
    uint64_t lane_clusters;          /* culling: cluster boxes that passed, per LANE (what each ray needs) */
    uint64_t lane_groups;            /* culling: outer boxes that passed, per LANE; range tables: window boxes reached */
    uint64_t group_maxpop;           /* culling: max over lanes of needed clusters, summed over visited groups */
    uint64_t query_maxpop;           /* culling: max over lanes of needed clusters, summed over wave-queries; grid: LANES whose
                                        origin lies beyond the lists' reach and that scan every clustered sphere
                                        (group_maxpop: lanes that walk the far tier of the lists) */
    uint64_t cycles[6];              /* shader-clock time per main-loop section, summed over waves: refill, prefix
                                        spheres, culled spheres + rects + cylinders, shading, accumulation, loop control */
    int32_t cull_prefix, cull_clusters, cull_groups, cull_cluster_size; /* table geometry */
    double wave_start_spread_us, wave_end_spread_us, wave_span_us; /* first-to-last wave start / exit, first start
                                        to last exit (s_memrealtime) */
    /* rt_render_hip_tiles only: kernel_ms above is the SLOWEST device's render launches */
    uint64_t lane_cands;  /* culling by range tables: candidate clusters per LANE before the per-cluster box test;
                             grid: cell steps per LANE (lane_groups = lanes that entered the grid, lane_clusters =
                             sphere tests per LANE); a step into or inside the sub-grid of a nested cell counts as a cell step */
    int32_t cull_mode;    /* candidate search of the kernel that ran: 5 uniform grid (6: its walk along x and z only, for a
                             grid one cell high; 7: over the wide tables; 8: over wide tables with nested cells), 3 range tables, 2 box hierarchy per lane, 1 wave votes, 0 none (flat scan) */
    int32_t cull_windows; /* windows of 64 clusters */
    double gather_ms;     /* root device: end of its own render -> assembled frame (ncclGather + row placement,
                             includes waiting for slower peers) */
    int32_t devices_used;
    int32_t grid_sheet;   /* rt_render_hip_count: 1 if the scene's grid is one cell high, i.e. the default kernel walks it along
                             x and z only (variant 2; the counting kernel itself walks in 3-D: same cells, same tests) */
    int32_t kernel_variant; /* the kernel that ran: what variant 0 (or a counting call) resolved to */
    int32_t walk_resumed; /* rt_render_hip_count, grid: LANES that took up a walk which the wave had cut short an iteration earlier
                             (its stragglers' hand-over; saturates at INT32_MAX).  In what was the struct's tail padding: same size */
} rt_stats;

void rt_opts_default(rt_opts *o);

/* number of image rows / floats a shard owns (dense local buffer:
 * local row r <-> global row rt_shard_row(...)). */
int rt_shard_rows(const rt_scene *s, const rt_opts *o);
int rt_shard_global_row(const rt_scene *s, const rt_opts *o, int local_row);
/* the value of rt_opts.tile_rotate that rt_render_hip_tiles uses to cut this frame (o: tile_rows) into n_ranks shards
 * (blue.py:23-32 deals whole frames to GPUs; here the tiles of one frame) */
int rt_shard_deal(const rt_scene *s, const rt_opts *o, int n_ranks);

/* render<<<grid, 8x8>>>(spp, background, cam, world, max_depth, W, H, image, states)
 * gpu-version/main.cu:72-105 with its launch at :505-507.
 * d_rgb_sum: DEVICE pointer, rt_shard_rows()*W*3 floats, local rows dense.
 * stream: hipStream_t as void* (NULL = default stream). Asynchronous when
 * stats == NULL; with stats it records hipEvents and synchronises the stream.
 * One scene object keeps one set of device accumulators per device: overlapping
 * renders of the SAME rt_scene on one device must be issued on the same stream
 * (use rt_scene_clone for independent concurrent frames). */
int rt_render_hip_device(const rt_scene *s, const rt_opts *o, void *d_rgb_sum, void *stream,
                         rt_stats *stats);

/* same, host buffer in / out: allocates, launches, copies back, frees
 * (main.cu:482-513: cudaMallocManaged + render + cudaDeviceSynchronize). */
int rt_render_hip(const rt_scene *s, const rt_opts *o, float *rgb_sum, rt_stats *stats);

/* One frame on n_devices GPUs of this node (SURVEY.md 8(b) "Threading", 8(e); the reference's only multi-GPU
 * mechanism is one renderer process per GPU per animation FRAME, gpu-version/blue.py:23-32).  The row tiles
 * (o->tile_rows rows, default 8) are dealt out as rt_shard_deal() says; devices[r] renders shard r on a stream of
 * its own -- the launch rt_render_hip_device makes for that shard -- then ONE ncclGather (rccl.h:745, root =
 * devices[0]) collects the dense local buffers and a kernel on the root places the rows; rgb_sum (host, H*W*3
 * floats) receives the frame.  The result is bit-identical to rt_render_hip for every n.  devices == NULL means
 * ordinals 0..n-1; the list must not repeat a device.  o->device, tile_first, tile_stride and tile_rotate are
 * ignored (the call sets them per device).
 * Streams, RCCL communicators (ncclCommInitAll, ~0.1 s once per device list) and buffers are kept between calls;
 * rt_tiles_shutdown() releases them.  RCCL is loaded with dlopen at the first call: librtmi.so does not link it. */
int rt_render_hip_tiles(const rt_scene *s, const rt_opts *o, const int *devices, int n_devices,
                        float *rgb_sum, rt_stats *stats);
void rt_tiles_shutdown(void);

/* diagnostic launch of the same kernel with exact event counters (samples,
 * hit queries, primitive tests, ...) for the roofline's algorithmic flops.
 * rgb_sum may be NULL. */
int rt_render_hip_count(const rt_scene *s, const rt_opts *o, float *rgb_sum, rt_stats *stats);

/* Progressive / resumable rendering (the reference's only analogue is the running
 * average of the Taichi renderers, taichi-version/4_0_path_tracing.py).  `acc` is the caller's
 * exact pixel sums for this shard, [local_rows][width][3] signed 64-bit fixed point in units of
 * 2^-24 (zero-initialised before the first call; a sample is clamped to +-2^16 and at most 2^23 samples per
 * pixel are accepted, so the sums never wrap).  The call adds the samples
 * [sample_first, sample_first + sample_count) of `o` to it; integer addition is exact and
 * commutative, so any split of a sample range into calls, processes or devices gives the same
 * sums -- and the same framebuffer -- as one rt_render_hip call over the whole range.
 * If rgb_sum is not NULL it receives the fp32 framebuffer of the updated sums. */
int rt_render_hip_accumulate(const rt_scene *s, const rt_opts *o, int64_t *acc, float *rgb_sum,
                             rt_stats *stats);

/* fractional bits of the exact pixel sums (a file or buffer of sums written in another scale cannot be continued) */
#define RT_ACC_FIX_BITS 24
/* fp32 framebuffer values of exact sums: rgb_sum[i] = (float)(acc[i] * 2^-24), the conversion the
 * render path itself applies once per launch. */
void rt_acc_to_rgb(const int64_t *acc, float *rgb_sum, size_t n_values);

/* scatter a shard's dense local rows into a full-image buffer (host side of
 * the multi-GPU gather; also used after the RCCL gather on the root). */
int rt_shard_scatter_rows(const rt_scene *s, const rt_opts *o, const float *local_rgb,
                          float *full_rgb);

/* the same on the device, for a GATHERED buffer: d_gathered[n_ranks][pad_rows][W][3] holds rank r's dense local
 * rows (o->tile_rotate says how the shards were cut -- which rank owns tile t of the frame and as which of its
 * local tiles; pad_rows >= the largest shard), as
 * ncclGather delivers them; one kernel on `stream` (hipStream_t as void*) writes d_full[H][W][3].
 * rt_render_hip_tiles uses it on its root device. */
int rt_shard_place_rows_device(const rt_scene *s, const rt_opts *o, int n_ranks, int pad_rows,
                               const void *d_gathered, void *d_full, void *stream);

/* ---- output ------------------------------------------------------------ */

/* output_image(), gpu-version/main.cu:359-372 + write_color color.cuh:70-95:
 * "P3\n%d %d\n255\n" then "%d %d %d\n" per pixel, rows top to bottom,
 * value = int(256 * clamp(sqrt(sum/spp), 0, 0.999)). */
int rt_write_ppm(const char *path, const float *rgb_sum, int width, int height, int spp);
/* the same quantisation into a caller buffer of width*height*3 bytes, rows top
 * to bottom; gamma = 0 gives write_image()'s linear bytes (color.cuh:15-35). */
int rt_quantize_rgb8(const float *rgb_sum, int width, int height, int spp, int gamma,
                     uint8_t *out);

/* write_image(), gpu-version/color.cuh:15-35 (called at main.cu:514 with json["output_file"]):
 * 8-bit RGB PNG, rows top to bottom; gamma = 0 is the reference's linear image. */
int rt_write_png(const char *path, const float *rgb_sum, int width, int height, int spp, int gamma);
/* the same two files from bytes that are already quantised (width*height*3, rows top to bottom: what rt_quantize_rgb8 and
 * rt_display_hip's out_rgb8 hold); rt_write_ppm and rt_write_png quantise and then go through these */
int rt_write_ppm_rgb8(const char *path, const uint8_t *rgb8, int width, int height);
int rt_write_png_rgb8(const char *path, const uint8_t *rgb8, int width, int height);
/* the scene's "output_file" (parser.hpp:566-567, default "main.png") */
const char *rt_scene_output_file(const rt_scene *s);

/* ---- misc -------------------------------------------------------------- */
const char *rt_last_error(void);
const char *rt_status_string(int status);
int rt_abi_version(void);
/* sizeof of the ABI structs as this library was compiled (binding self-checks):
 * 0 rt_opts, 1 rt_stats, 2 rt_prim, 3 rt_material, 4 rt_texture, 5 rt_camera, 6 rt_scene_info, 7 rt_table_info,
 * 8 rt_adaptive, 9 rt_adaptive_stats, 10 rt_nested_info, 16 rt_denoise, 17 rt_medium, 18 rt_moving_sphere, 19 rt_display,
 * 20 rt_display_stats, 21 rt_ray, 22 rt_hit, 24 rt_noise, 25 rt_analytic_light; else 0 */
size_t rt_struct_size(int which);
/* number of usable gfx950 devices, or -rt_status */
int rt_device_count(void);
/* 1 if this library carries the measurement variants of rt_opts.variant and the counting kernels of rt_render_hip_count
 * (the default build; `make ABLATIONS=0` builds the six product kernels alone: same ABI, rt_render_hip_count then
 * fails with RT_ERR_LIMIT and rt_opts.variant accepts 0, 2, 6, 16, 36, 44, 52) */
int rt_has_ablations(void);
/* The workgroup that render variant `variant` (never 0) launches, as the host sizes it; no device is touched.
 * out[0] threads per workgroup, out[1] bytes of LDS per wave behind the staged tables (tile accumulator; variants 2 and 6:
 * and the slab of prepared camera rays), out[2] the largest table size in bytes that the packer keeps LDS-resident,
 * out[3] dynamic LDS in bytes of a workgroup that stages tables of that size, out[4] workgroups per CU that the kernel's
 * registers and the wave slots admit (what the LDS of a CU, 160 KB, has to hold).  RT_ERR_ARG for a null pointer or a variant
 * this library does not carry. */
int rt_variant_workgroup(unsigned variant, int32_t out[5]);
/* Philox4x32-10 block (seeds every (pixel, sample) stream), for known-answer tests */
void rt_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* first n raw 32-bit words of the xorshift128 stream of one (pixel, sample); the kernel's
 * uniforms are (word >> 8) * 2^-24 */
void rt_sample_stream(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t *out, int n);
/* slab test, gpu-version/aabb.hpp:15-29 (host evaluation of the device helper's formula) */
int rt_aabb_hit(const float bmin[3], const float bmax[3], const float orig[3], const float dir[3],
                float t_min, float t_max);

/* ---- adaptive sampling --------------------------------------------------- */

/* Per-tile sample counts driven by a noise target.  Every 8x8 tile starts with min_spp samples; after each pass a
 * tile whose noise estimate is within `threshold` (or that has reached max_spp) is retired and the others double
 * their samples: n_0 = min_spp, n_{k+1} = min(2 n_k, max_spp).  The samples of a pass go half to one accumulator
 * plane (A) and half to another (B); the noise of a pixel is estimated from the two half-sums, in fp64:
 *     a_c = SA_c 2^-24 / nA,  b_c = SB_c 2^-24 / nB,  m_c = (SA_c + SB_c) 2^-24 / n
 *     d = (|a_r - b_r| + |a_g - b_g|) + |a_b - b_b|,  M = max((m_r + m_g) + m_b, 1e-4)
 *     converged  <=>  d * d <= (4 T T) M              (d / (2 sqrt M) <= T)
 * and a tile converges when all its on-image pixels do.  threshold = 0 retires tiles at max_spp only.
 * A tile that stops after n samples holds exactly the sums of samples [0, n): bit for bit what rt_render_hip gives
 * that tile at spp = n. */
typedef struct rt_adaptive {
    int32_t min_spp;    /* samples of the first pass, every tile; >= 2 */
    int32_t max_spp;    /* cap per tile; 0 -> the scene's spp; >= min_spp */
    float   threshold;  /* noise target (metric above); >= 0 and finite; 0 -> every tile runs to max_spp */
} rt_adaptive;

typedef struct rt_adaptive_stats {
    int32_t passes;
    int32_t tiles;            /* 8x8 tiles of the frame */
    int32_t spp_after[32];    /* n_k: samples per active tile after pass k */
    int32_t active[32];       /* tiles rendered in pass k */
    uint64_t samples;         /* pixel samples rendered: sum of spp_map over on-image pixels */
    double kernel_ms;         /* render + estimate kernels, hipEvent time */
} rt_adaptive_stats;

/* rgb_sum (host, H*W*3 floats): rgb_sum[(y*W+x)*3+c] is the fp32 conversion of the pixel's exact sum over its own
 * spp_map[y*W+x] samples [0, n) (host, H*W int32).  The whole frame on o->device; o->tile_stride must be <= 1 and
 * o->sample_first / sample_count 0 (the schedule owns the samples).  o->variant: 0 or any rendering variant.  Light
 * sampling follows the scene's switch.  RT_ERR_ARG for bad arguments, checked before any device access; st may be NULL. */
int rt_render_hip_adaptive(const rt_scene *s, const rt_opts *o, const rt_adaptive *a,
                           float *rgb_sum, int32_t *spp_map, rt_adaptive_stats *st);
/* the same into DEVICE buffers on `stream` (hipStream_t as void*); returns when the frame is done (the schedule reads the
 * active tile count back once per pass) */
int rt_render_hip_adaptive_device(const rt_scene *s, const rt_opts *o, const rt_adaptive *a,
                                  void *d_rgb_sum, void *d_spp_map, void *stream, rt_adaptive_stats *st);

/* ---- first-hit feature buffers and the denoiser --------------------------- */

/* A feature sample is an ordinary sample up to its first closest-hit query: the same (seed, pixel, sample) stream, jitter,
 * lens draw, camera ray and candidate search.  There the path ends and, in place of radiance, adds one triple to the
 * pixel's exact fixed-point sum (no Russian-roulette draw, no light sample, no scatter; max_depth plays no part):
 *   RT_FEATURE_ALBEDO  hit: lambertian / diffuse_light: the texture's value at the hit (solid, checker, image); metal: albedo;
 *                           dielectric: (1, 1, 1).  miss: what the miss gives a fresh path (sky gradient or background)
 *   RT_FEATURE_NORMAL  hit: the hit record's normal, turned against the ray (not re-normalised).  miss: (0, 0, 0)
 *   RT_FEATURE_DEPTH   hit: (t of the hit record, 1, 0).  miss: (0, 0, 0) -- channel 1 sums to the samples that hit (coverage)
 * The albedo pass of a scene is therefore, bit for bit, the render of its clone whose every material is a diffuse_light
 * on the same texture. */
typedef enum rt_feature {
    RT_FEATURE_ALBEDO = 0,
    RT_FEATURE_NORMAL = 1,
    RT_FEATURE_DEPTH = 2
} rt_feature;

/* One feature pass: `sum` (host, rt_shard_rows()*W*3 floats, local rows dense, as rt_render_hip) receives the fp32
 * conversion of the exact sums over samples [o->sample_first, + o->sample_count) (0 -> the scene's spp).  Honours the shard
 * fields and spp_chunk like rt_render_hip; every split of a sample range and every row shard composes exactly.
 * o->variant names the LAYOUT: 0 (the scene's default), 16 / 24 (linear scan, tables in LDS / global memory), 36 / 44 (wide
 * grid walk) or 52 (nested walk); a scene with compact tables (variants 2, 6) runs the linear scan, in LDS while it fits and
 * from global memory beyond (no size limit); every layout gives the same bytes.  Other variants fail with RT_ERR_ARG.  Light
 * sampling and Russian roulette do not bear on a feature.  rt_stats.kernel_variant reports the layout | 512.
 * A scene with an environment map: the albedo pass gives the map's radiance on a miss (what the miss gives a fresh path), normal
 * and depth give zeros; layouts 0, 16, 36 and 44 (the layout | 512 | 1024).
 * RT_ERR_ARG for a null pointer or a feature outside 0..2, checked before any device access; stats may be NULL. */
int rt_render_hip_feature(const rt_scene *s, const rt_opts *o, int feature, float *sum, rt_stats *stats);
/* the same into a DEVICE buffer on `stream` (hipStream_t as void*), asynchronous when stats == NULL (rt_render_hip_device) */
int rt_render_hip_feature_device(const rt_scene *s, const rt_opts *o, int feature, void *d_sum, void *stream,
                                 rt_stats *stats);

/* ---- ray queries: closest hit and occlusion for caller-supplied rays ---------------------------------
 *
 * A ray query is exactly the renderer's closest-hit query: hittable_list::hit over the scene's STATIC primitives in list
 * order, over the range [0.001, t_max]; a hit with t <= the closest so far is accepted, so at equal t the later list entry
 * wins.  dir is not normalised and t is in units of dir; t_max = +inf is allowed, a negative t_max is valid and misses.
 * The walk is the render kernels' own (one 3-D DDA over the scene's tables, bit-identical to the linear scan in every
 * layout), and the record carries what their winner section computes:
 *   hit      t, point (p = o + t d as the kernels evaluate it, fp32; a cylinder's through its object space), the hit record's
 *            normal turned against the ray, front (1: the ray met the outward side), the material index, prim (the index into
 *            rt_scene_get_prims) and the hit record's (u, v), evaluated for EVERY hit here by the fixed atan2 / acos sequences
 *            the image textures are read with (the render kernels evaluate them for image textures only)
 *   miss     t = +inf, prim = -1, every other word 0
 *   invalid  prim = RT_HIT_INVALID, t = +inf, every other word 0.  A ray is invalid if a component of origin or dir is not
 *            finite, t_max is NaN, or dir.dir evaluated in fp32 (fma(dx, dx, fma(dy, dy, dz dz))) is zero, denormal or not
 *            finite.  Such a ray never enters the walk.  rt_ray_valid is the host evaluation of the kernel's guard.
 * RT_TRACE_OCCLUDED writes one uint8_t per ray instead: 1 iff RT_TRACE_CLOSEST would report a hit for the same ray, else 0
 * (an invalid ray: 0).  out[i] belongs to ray i; its bytes do not depend on n, on the batch the ray arrives in, on the
 * layout or on the schedule.  `reserved` is ignored.
 * What a query sees: the static primitives.  Media and an environment map are not surfaces and are ignored (as feature
 * passes ignore media); light sampling, Russian roulette, max_depth, the frame size and the camera play no part.  A scene
 * with moving spheres is refused with RT_ERR_ARG (a query has no shutter time: clear the movers, rt_scene_clear_moving_spheres).
 * rt_opts: `device` and `variant` are read, every other field is ignored.  variant names the LAYOUT as for
 * rt_render_hip_feature: 0, 16, 24, 36, 44 or 52; a scene with compact tables runs the linear scan, in LDS while it fits and
 * from global memory beyond; any other variant is RT_ERR_ARG.  rt_stats reports kernel_ms, upload_ms and launches, and
 * kernel_variant the layout | 8192.
 * Errors, all checked before any device access: null scene, a mode outside 0..1, a variant outside the list, moving
 * spheres: RT_ERR_ARG; n >= 2^31: RT_ERR_LIMIT; n == 0 returns RT_OK without touching a device; null rays or null out with
 * n > 0: RT_ERR_ARG. */
typedef struct rt_ray { float origin[3]; float t_max; float dir[3]; float reserved; } rt_ray;   /* 32 bytes: two 16-byte records */
typedef struct rt_hit {                     /* 48 bytes: three 16-byte records */
    float t; int32_t prim; int32_t material; int32_t front;
    float normal[3]; float u;
    float point[3];  float v;
} rt_hit;
#define RT_HIT_INVALID (-2)
typedef enum rt_trace_mode { RT_TRACE_CLOSEST = 0, RT_TRACE_OCCLUDED = 1 } rt_trace_mode;
/* rays per work item of the query kernels: scheduling only, it bears on no record (exposed for the tests' batch sizes) */
#define RT_TRACE_ITEM 64
/* rays (host, n records) -> out (host: n rt_hit, or n bytes in occlusion mode); stats may be NULL */
int rt_trace_hip(const rt_scene *s, const rt_opts *o, int mode, const rt_ray *rays, size_t n, void *out, rt_stats *stats);
/* the same on DEVICE buffers (16-byte aligned) on `stream` (hipStream_t as void*), asynchronous when stats == NULL
 * (rt_render_hip_device); the scene's tables are uploaded and cached per device as for a render.  Queries and renders of ONE
 * scene object on one device must share a stream, or be serialised by the caller (they share its tables and work counter);
 * different scene objects, or clones, are independent */
int rt_trace_hip_device(const rt_scene *s, const rt_opts *o, int mode, const void *d_rays, size_t n, void *d_out, void *stream, rt_stats *stats);
/* 1: the ray may enter the walk; 0: it is invalid (or r is NULL).  No GPU needed. */
int rt_ray_valid(const rt_ray *r);
/* Host evaluation of the scene's camera, any projection (rt_scene_set_projection; no GPU needed): the ray the kernels start at
 * (s, t) for the lens sample (lx, ly) of the unit disk, from the fp32 camera records the device reads, operation for
 * operation (csrc/rt_camera.h; the sines and cosines come from the host's math library).  The lens sample acts iff the scene
 * has RT_FLAG_DEFOCUS_BLUR, as in a render.  out->t_max = +inf.  *valid (may be NULL) = 1, or 0 where the projection has no ray
 * -- a fisheye sample outside the image circle: *out is then zeros with t_max = +inf, which rt_ray_valid refuses too. */
int rt_camera_ray(const rt_scene *s, float sx, float t, float lx, float ly, rt_ray *out, int *valid);

/* ---- the denoiser (guided by the first-hit feature buffers above) ------------ */

/* Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on the demodulated image (mean colour / first-hit albedo),
 * guided by the three feature sums.  The definition -- prepare, weights, order of the taps, pixels without coverage -- is
 * DESIGN.md section 7d; every operation in it is a single fp32 + - x / min max in a fixed order, so a numpy float32
 * restatement reproduces the output bit for bit.
 * A sigma of 0 means its default (sigma_color 0.5, sigma_normal 0.125, sigma_depth 0.05: measured).  iterations counts the passes, pass i with
 * taps 2^i pixels apart: 0 .. 10, where 0 passes returns the input bits; RT_DENOISE_DEFAULT_ITERATIONS (-1) means the
 * default, 3 -- as does a NULL rt_denoise, which is all defaults.  (0 cannot stand for both "no pass" and "the default":
 * for this one field the default has a value of its own.)  rt_struct_size(16) reports sizeof(rt_denoise): index 11 and
 * its neighbours are left to the structs of the scene and render interface. */
#define RT_DENOISE_DEFAULT_ITERATIONS (-1)
typedef struct rt_denoise {
    int32_t iterations;   /* passes; 0 .. 10, or RT_DENOISE_DEFAULT_ITERATIONS                                    */
    float sigma_color;    /* colour term: |e - e'| of the demodulated colours against sqrt(l^2 + 1/16), l the centre's
                             r + g + b; halves from pass to pass                                                     */
    float sigma_normal;   /* normal term: |n - n'| of the mean normals                                               */
    float sigma_depth;    /* depth term: |t - t'| / t of the mean hit distances                                      */
} rt_denoise;

/* rgb_sum (host, H*W*3 floats): a frame of rt_render_hip over `spp` samples per pixel, or -- spp_map != NULL (H*W int32,
 * spp then ignored) -- a frame of rt_render_hip_adaptive with its per-pixel sample counts (an entry < 1 counts as 1).
 * albedo_sum, normal_sum, depth_sum: the three passes of rt_render_hip_feature over feature_spp samples each, whole frames.
 * out_rgb_sum (must not overlap an input) receives the filtered frame, again a SUM over the pixel's samples:
 * rt_write_ppm, rt_write_png and rt_quantize_rgb8 take it unchanged.  ms (may be NULL): hipEvent time of the kernels.
 * RT_ERR_ARG, checked before any device access, for: a null buffer, a size <= 0 (or > 65536), spp <= 0 without an spp_map,
 * feature_spp <= 0, a negative or non-finite sigma, iterations outside -1 .. 10. */
int rt_denoise_hip(int width, int height, const float *rgb_sum, int spp, const int32_t *spp_map, const float *albedo_sum,
                   const float *normal_sum, const float *depth_sum, int feature_spp, const rt_denoise *p, int device,
                   float *out_rgb_sum, double *ms);
/* the same on DEVICE buffers of device `device`, enqueued on `stream` (hipStream_t as void*); asynchronous when ms == NULL.
 * Scratch buffers (three planes of 16 bytes per pixel) are kept per device between calls: overlapping calls on one
 * device must share a stream. */
int rt_denoise_hip_device(int width, int height, const void *d_rgb_sum, int spp, const void *d_spp_map,
                          const void *d_albedo_sum, const void *d_normal_sum, const void *d_depth_sum, int feature_spp,
                          const rt_denoise *p, int device, void *d_out_rgb_sum, void *stream, double *ms);

/* ---- display stage: exposure, bloom, tone curve, 8-bit quantisation; HDR files ---------------------------------
 * Runs after the render (and after rt_denoise_hip where that is used) on a whole frame of sums.  The definition -- mean,
 * auto exposure from an exact integer log-luminance sum, scale, bloom as the mean of the smooth planes of a B3-spline a-trous
 * transform, tone curve, quantisation -- is DESIGN.md section 7i; every device operation in it is a single fp32 + - x / min
 * max sqrt in a fixed order (no exp / log / pow), so a numpy float32 restatement reproduces both outputs bit for bit. */
typedef enum rt_tonemap { RT_TONEMAP_CLAMP = 0, RT_TONEMAP_REINHARD = 1, RT_TONEMAP_ACES = 2 } rt_tonemap;
typedef struct rt_display {
    int32_t tonemap;          /* rt_tonemap */
    float   exposure;         /* linear multiplier > 0; 0 -> 1 */
    float   auto_key;         /* > 0: exposure is chosen from the frame (the log-average luminance is mapped to auto_key)
                                 and `exposure` multiplies it; 0: off */
    float   white;            /* Reinhard's white point > 0; 0 -> 4 */
    float   bloom_strength;   /* >= 0; 0: no bloom, no bloom kernels are launched */
    float   bloom_threshold;  /* >= 0; 0 is a valid value here, not a stand-in for a default; all-defaults is a NULL rt_display */
    int32_t bloom_levels;     /* 1 .. 8; 0 -> 5 */
} rt_display;
typedef struct rt_display_stats {
    int64_t log_sum;          /* auto exposure: sum over pixels of (bits of the clamped luminance) - 0x3F800000; 0 when off */
    float   exposure_used;    /* the multiplier E the pixels were scaled by */
    double  ms;               /* hipEvent time of the kernels */
} rt_display_stats;

/* rgb_sum, spp, spp_map: as for rt_denoise_hip (H*W*3 floats, row 0 at the bottom; an spp_map entry < 1 counts as 1).
 * out_rgb (H*W*3 floats, same layout): display-referred linear colour, a sum over ONE sample -- the writers take it with
 * spp = 1.  out_rgb8 (H*W*3 bytes, rows top to bottom): int(256 clamp(sqrt(out_rgb), 0, 0.999)), what
 * rt_quantize_rgb8(out_rgb, W, H, 1, 1, .) gives.  Either output may be NULL, not both.  p == NULL: all defaults (clamp,
 * E = 1, no bloom): out_rgb is rgb_sum / n, and out_rgb8 is what rt_quantize_rgb8(rgb_sum, W, H, spp, 1, .) writes -- whenever
 * the stage is ASKED to be this identity (p == NULL, or clamp with exposure 0 or 1, auto_key 0 and bloom_strength 0: a matter of
 * the parameters, never of a computed exposure) the byte is taken from the sum in the writer's own form, sqrt(rgb_sum x (1 / n)),
 * which can differ from sqrt(rgb_sum / n) -- the byte of out_rgb -- in the last bit.
 * RT_ERR_ARG, checked before any device access, for: a null input, both outputs null, a size <= 0 (or > 65536), spp <= 0
 * without an spp_map, a negative or non-finite field, tonemap outside 0 .. 2, bloom_levels outside 0 .. 8.  st may be NULL. */
int rt_display_hip(int width, int height, const float *rgb_sum, int spp, const int32_t *spp_map, const rt_display *p, int device,
                   float *out_rgb, uint8_t *out_rgb8, rt_display_stats *st);
/* the same on DEVICE buffers of device `device`, enqueued on `stream` (hipStream_t as void*); asynchronous when st == NULL and
 * auto_key == 0 (auto exposure reads its sum back once, which waits for the stream).  Scratch buffers (four planes of 16 bytes
 * per pixel) are kept per device between calls: overlapping calls on one device must share a stream. */
int rt_display_hip_device(int width, int height, const void *d_rgb_sum, int spp, const void *d_spp_map, const rt_display *p,
                          int device, void *d_out_rgb, void *d_out_rgb8, void *stream, rt_display_stats *st);
/* A measuring hook, not part of the stage's interface (tools/gpu_display.py reads it; nothing else needs it): the
 * hipEvent times (ms) of the single kernels of this thread's last rt_display_hip* call that had st != NULL, in launch order:
 * [reduction (auto exposure only),] prepare, [blur level 0 horizontal, vertical, level 1 ...,] finish.  Copies at most cap
 * entries; returns the number of kernels. */
int rt_display_timing(double *ms, int cap);

/* The MEAN image rgb_sum / spp -- scene-referred: no exposure, no curve -- as a float image file.  Both are read back by
 * rt_scene_set_environment_file with the image's top row as the zenith row.  RT_ERR_ARG / RT_ERR_IO as the other writers.
 * rt_write_hdr: Radiance RGBE, "-Y H +X W", rows top to bottom, flat scanlines; the exponent comes from the largest channel
 * and mantissas are truncated (negative and NaN channels are written as 0).
 * rt_write_pfm: "PF", scale -1.0 (little-endian), rows bottom to top: the framebuffer's own order. */
int rt_write_hdr(const char *path, const float *rgb_sum, int width, int height, int spp);
int rt_write_pfm(const char *path, const float *rgb_sum, int width, int height, int spp);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_H */
