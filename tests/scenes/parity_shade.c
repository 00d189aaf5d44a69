/* parity_shade.c -- a scene program written for this repository's shading tests (original code,
 * ndt scene API: scene_setup(scene*, dims, frame, frames, config)).
 *
 * One small frame of it takes every branch of the reference's apply_lights, get_ray_color and
 * vectNd_refract (ndt.c:71-450, vectNd.c:119-188) in every dimension 3 .. 12; which branches, and how
 * often each must be taken, is counted and asserted in tests/test_shading_known_answers.py.  Only
 * cheap objects: spheres, an hplane, hdisks, one hcylinder.  Compiled against the REFERENCE's headers
 * by oracle/Makefile (-> oracle/_ref/scenes/parity_shade.so) for tests/golden/make_golden_shade.py.
 *
 *   floor       hplane through the origin, normal (0,-1,0,...): viewer and lights stand on its negative
 *               side, so it is lit WITHOUT the `angle = PI - angle` flip; its reflectance's maximum is blue
 *   window      glass hdisk, reflectance 0, seen from its negative-normal side at 23 .. 40 degrees: index
 *               inverted, total internal reflection on one part and refraction out on the other
 *   weak ball   glass sphere, reflectance (0.05, 0.15, 0.1), a point light inside: the chain of inside
 *               reflections dies at the 1/512 weight; inside hits see their own far wall in the shadow ray
 *   strong ball glass sphere, reflectance (0.9, 0.6, 0.3): the chain of inside reflections dies at the depth limit
 *   mirror ball opaque, reflectance (0, 0.3, 0): two zero channels, maximum green; on the spot cone's edge
 *   pillar      opaque finite hcylinder (a curved N-D normal), on the spot cone's edge
 *   wall        opaque hdisk behind, no reflectance: a hit without children
 *   lights      an ambient entry; a point light (green brightest); the point light in the weak ball (blue);
 *               a far spot light (blue) with a 2.5 degree cone, so that half a degree is a pixel wide; a
 *               directional light (red); a directional light whose direction lies IN the floor's hyperplane
 *               (component 1 is 0.0: rev_light . normal is a sum of zeros for every floor hit, the same-side
 *               product is exactly 0); a point light 2^-10 above the floor, whose shadow rays the floor's
 *               intersector turns away (|v . n| <= EPSILON) beyond ten units: they find nothing at all
 */
#include <stdio.h>
#include <string.h>
#include "../scene.h"

static void set_axis(vectNd *v, int dims, double a0, double a1, double a2, double rest)
{
    vectNd_reset(v);
    vectNd_set(v, 0, a0);
    vectNd_set(v, 1, a1);
    vectNd_set(v, 2, a2);
    for (int i = 3; i < dims; ++i) vectNd_set(v, i, rest * (1.0 + 0.25 * (i - 3)));
}

static object *add(scene *scn, int dims, char *type, double r, double g, double b, double rr, double gr, double br)
{
    object *o = NULL;
    scene_alloc_object(scn, dims, &o, type);
    o->red = r; o->green = g; o->blue = b;
    o->red_r = rr; o->green_r = gr; o->blue_r = br;
    return o;
}

static light *add_light(scene *scn, int dims, int type, double r, double g, double b)
{
    light *l = NULL;
    scene_alloc_light(scn, &l);
    l->type = type;
    l->red = r; l->green = g; l->blue = b;
    if (type == LIGHT_POINT || type == LIGHT_SPOT) vectNd_calloc(&l->pos, dims);
    if (type == LIGHT_DIRECTIONAL || type == LIGHT_SPOT) vectNd_calloc(&l->dir, dims);
    return l;
}

int scene_frames(int dimensions, char *config)
{
    (void)dimensions; (void)config;
    return 1;
}

int scene_setup(scene *scn, int dims, int frame, int frames, char *config)
{
    (void)frame; (void)frames; (void)config;
    scene_init(scn, "parity_shade", dims);
    scn->bg_red = 0.1; scn->bg_green = 0.05; scn->bg_blue = 0.2; scn->bg_alpha = 0.5;
    scn->ambient.red = 0.04; scn->ambient.green = 0.05; scn->ambient.blue = 0.03;

    vectNd p, q, d;
    vectNd_calloc(&p, dims);
    vectNd_calloc(&q, dims);
    vectNd_calloc(&d, dims);

    camera_reset(&scn->cam);
    set_axis(&p, dims, 2.0, 18.0, 46.0, 0.2);
    set_axis(&q, dims, 0.0, 3.0, 2.0, 0.1);
    vectNd_reset(&d);
    vectNd_set(&d, 1, 1.0);
    camera_set_aim(&scn->cam, &p, &q, &d, 0.0);

    light *l;
    add_light(scn, dims, LIGHT_AMBIENT, 0.06, 0.05, 0.08);

    l = add_light(scn, dims, LIGHT_POINT, 220, 260, 200);
    set_axis(&l->pos, dims, -6.0, 22.0, 16.0, 0.2);

    /* inside the weak ball (same offsets in the further dimensions as its centre) */
    l = add_light(scn, dims, LIGHT_POINT, 9, 7, 14);
    set_axis(&l->pos, dims, 10.0, 5.5, 4.0, 0.1);

    /* spot: 200 away from the floor point it looks at, 2.5 degrees */
    l = add_light(scn, dims, LIGHT_SPOT, 28000, 20000, 40000);
    set_axis(&l->dir, dims, -0.25, -1.0, -0.15, 0.02);
    vectNd_unitize(&l->dir);
    set_axis(&p, dims, 5.0, 0.0, 14.0, 0.0);
    vectNd_scale(&l->dir, -200.0, &q);
    vectNd_add(&p, &q, &l->pos);
    l->angle = 2.5;

    l = add_light(scn, dims, LIGHT_DIRECTIONAL, 0.5, 0.3, 0.2);
    set_axis(&l->dir, dims, -0.4, -1.0, -0.5, -0.1);

    /* in the floor's hyperplane: component 1 is exactly 0 */
    l = add_light(scn, dims, LIGHT_DIRECTIONAL, 0.2, 0.25, 0.15);
    set_axis(&l->dir, dims, 1.0, 0.0, -0.5, 0.2);

    /* 2^-10 above the floor */
    l = add_light(scn, dims, LIGHT_POINT, 3, 3, 2);
    set_axis(&l->pos, dims, -2.0, 0.0009765625, 24.0, 0.0);

    object *o;
    /* floor: through the origin, normal pointing down */
    o = add(scn, dims, "hplane", 0.7, 0.7, 0.65, 0.1, 0.2, 0.4);
    vectNd_reset(&p);
    object_add_pos(o, &p);
    set_axis(&d, dims, 0.0, -1.0, 0.0, 0.0);
    object_add_dir(o, &d);

    /* window: the camera is on its negative-normal side */
    o = add(scn, dims, "hdisk", 0.3, 0.8, 0.4, 0.0, 0.0, 0.0);
    o->transparent = 1;
    o->refract_index = 1.9;
    set_axis(&p, dims, -11.0, 7.0, 10.0, 0.1);
    object_add_pos(o, &p);
    set_axis(&d, dims, 0.218, -0.276, -0.936, -0.01);
    vectNd_unitize(&d);
    object_add_dir(o, &d);
    object_add_size(o, 7.0);

    /* weak ball */
    o = add(scn, dims, "sphere", 0.9, 0.95, 1.0, 0.05, 0.15, 0.1);
    o->transparent = 1;
    o->refract_index = 1.45;
    set_axis(&p, dims, 10.0, 5.0, 4.0, 0.1);
    object_add_pos(o, &p);
    object_add_size(o, 4.5);

    /* strong ball */
    o = add(scn, dims, "sphere", 0.8, 0.9, 0.7, 0.9, 0.6, 0.3);
    o->transparent = 1;
    o->refract_index = 1.3;
    set_axis(&p, dims, -1.0, 5.0, 2.0, 0.05);
    object_add_pos(o, &p);
    object_add_size(o, 4.5);

    /* mirror ball */
    o = add(scn, dims, "sphere", 0.9, 0.2, 0.2, 0.0, 0.3, 0.0);
    set_axis(&p, dims, 11.5, 3.5, 15.0, 0.15);
    object_add_pos(o, &p);
    object_add_size(o, 3.5);

    /* pillar: finite hcylinder (flag[0] = 0), dims-1 positions */
    o = add(scn, dims, "hcylinder", 0.6, 0.2, 0.7, 0.1, 0.1, 0.1);
    object_add_flag(o, 0);
    set_axis(&p, dims, -1.5, 0.5, 15.0, -0.1);
    object_add_pos(o, &p);
    for (int i = 0; i < dims - 2; ++i) {
        vectNd_copy(&q, &p);
        vectNd_set(&q, (i == 0) ? 1 : i + 1, q.v[(i == 0) ? 1 : i + 1] + 6.0 + i);
        vectNd_set(&q, 0, q.v[0] + 0.25 * (i + 1));
        object_add_pos(o, &q);
    }
    object_add_size(o, 1.5);

    /* wall: behind everything, its normal pointing away */
    o = add(scn, dims, "hdisk", 0.8, 0.8, 0.5, 0.0, 0.0, 0.0);
    set_axis(&p, dims, 0.0, 8.0, -12.0, 0.0);
    object_add_pos(o, &p);
    set_axis(&d, dims, 0.0, 0.0, -1.0, 0.0);
    object_add_dir(o, &d);
    object_add_size(o, 14.0);

    vectNd_free(&p);
    vectNd_free(&q);
    vectNd_free(&d);
    return 1;
}

int scene_cleanup(void) { return 0; }
