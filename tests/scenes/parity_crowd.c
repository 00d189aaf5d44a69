/* parity_crowd.c -- a scene program written for this repository's trace-tier tests (original code, ndt scene API:
 * scene_setup(scene*, dims, frame, frames, config)).
 *
 * The zoo (parity_zoo.c) has every object type but only 13 to 15 items: it never leaves the item-set kernels.  This scene
 * is a CROWD: one floor hplane and K - 1 small objects that cycle through the other eight types, so that every 64-item
 * word of a visit mask holds every type, for any dims >= 3.  The objects stand on a jittered lattice in a box in front of
 * the camera, with skewed directions; their bounding boxes reach into the neighbouring cells, so the kd builder's leaves
 * share items.  About one object in eight is reflective, one in eight is glass; the zoo's four kinds of light are here.
 * Everything follows from the arguments through a small integer generator of its own.
 *
 * config: "items=K" (default 320), "seed=S" (default 1), "nohcube" (no hcube: it nests every m-face, 52 904 of them in
 * 10-D), "mix=light" / "mix=spheres" (the K - 1 small objects cycle through the three types with the shortest records --
 * sphere, hdisk, cylinder -- or are all spheres, placed the same way: 192 and 256 items within a 64 KB trace section; no
 * hcube).  Without nohcube the crowd holds two hcubes up to 6-D and one above, in different mask words.
 * Compiled against the REFERENCE's headers by oracle/Makefile (-> oracle/_ref/scenes/parity_crowd.so).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "../scene.h"

static unsigned long long crowd_state;

static unsigned int rnd(void)
{
    crowd_state = crowd_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (unsigned int)(crowd_state >> 33);
}

/* uniform in [lo, hi) */
static double uni(double lo, double hi) { return lo + (hi - lo) * (rnd() / 2147483648.0); }

static int config_int(char *config, const char *key, int fallback)
{
    char *at = config ? strstr(config, key) : NULL;
    return at ? atoi(at + strlen(key)) : fallback;
}

/* a vector of the given length with no zero component, in no axis' direction */
static void skew_vec(vectNd *v, int dims, double len)
{
    for (int i = 0; i < dims; ++i) {
        double c = uni(0.2, 1.0);
        vectNd_set(v, i, (rnd() & 1) ? c : -c);
    }
    vectNd_unitize(v);
    vectNd_scale(v, len, v);
}

/* a: what is left of it after its part along unit vector u is taken away */
static void remove_part(vectNd *a, vectNd *u, int dims)
{
    double dot = 0.0;
    for (int i = 0; i < dims; ++i) dot += a->v[i] * u->v[i];
    for (int i = 0; i < dims; ++i) vectNd_set(a, i, a->v[i] - dot * u->v[i]);
}

static void offset(vectNd *out, vectNd *c, vectNd *d, double s, int dims)
{
    for (int i = 0; i < dims; ++i) vectNd_set(out, i, c->v[i] + s * d->v[i]);
}

int scene_frames(int dimensions, char *config)
{
    (void)dimensions; (void)config;
    return 1;
}

int scene_setup(scene *scn, int dims, int frame, int frames, char *config)
{
    (void)frame; (void)frames;
    const int items = config_int(config, "items=", 320);
    const int light_mix = (config && strstr(config, "mix=light")) ? 3 : (config && strstr(config, "mix=spheres")) ? 1 : 0;
    const int nohcube = (light_mix || (config && strstr(config, "nohcube"))) ? 1 : 0;
    crowd_state = 0x9E3779B97F4A7C15ULL ^ ((unsigned long long)config_int(config, "seed=", 1) << 20) ^ (unsigned long long)dims;
    for (int i = 0; i < 4; ++i) rnd();

    scene_init(scn, "parity_crowd", dims);
    scn->bg_red = 0.04; scn->bg_green = 0.08; scn->bg_blue = 0.16; scn->bg_alpha = 0.5;
    scn->ambient.red = 0.05; scn->ambient.green = 0.04; scn->ambient.blue = 0.03;

    vectNd c, p, d, e;
    vectNd_calloc(&c, dims);
    vectNd_calloc(&p, dims);
    vectNd_calloc(&d, dims);
    vectNd_calloc(&e, dims);

    /* the lattice: g x h x g cells of the first three coordinates, the box centred on the y axis, its lowest cells above the floor */
    const int count = items - 1;
    int g = 1;
    while (g * g * g < count) ++g;
    int h = (count + g * g - 1) / (g * g);
    const double pitch = 1.8, floor_y = -6.0, base_y = -2.5;

    /* camera: off-axis in every dimension, looking down into the box */
    camera_reset(&scn->cam);
    vectNd_reset(&p);
    vectNd_reset(&c);
    for (int i = 0; i < dims; ++i) vectNd_set(&p, i, i == 0 ? 1.9 * g * pitch : i == 1 ? 14.0 : i == 2 ? 1.5 * g * pitch : 1.5 + 0.4 * (i - 3));
    vectNd_set(&c, 1, base_y + 0.4 * h * pitch);
    vectNd_reset(&d);
    vectNd_set(&d, 1, 1.0);
    camera_set_aim(&scn->cam, &p, &c, &d, 0.05);

    /* lights: ambient entry, point, spot, directional */
    light *l = NULL;
    scene_alloc_light(scn, &l);
    l->type = LIGHT_AMBIENT;
    l->red = 0.08; l->green = 0.08; l->blue = 0.1;

    scene_alloc_light(scn, &l);
    l->type = LIGHT_POINT;
    vectNd_calloc(&l->pos, dims);
    for (int i = 0; i < dims; ++i) vectNd_set(&l->pos, i, i == 0 ? 6.0 : i == 1 ? 26.0 : i == 2 ? 11.0 : 1.0 + 0.3 * (i - 3));
    l->red = 300; l->green = 280; l->blue = 240;

    scene_alloc_light(scn, &l);
    l->type = LIGHT_SPOT;
    vectNd_calloc(&l->pos, dims);
    vectNd_calloc(&l->dir, dims);
    for (int i = 0; i < dims; ++i) {
        vectNd_set(&l->pos, i, i == 0 ? -8.0 : i == 1 ? 30.0 : i == 2 ? 3.0 : -0.5);
        vectNd_set(&l->dir, i, i == 0 ? 0.25 : i == 1 ? -1.0 : i == 2 ? -0.1 : 0.02);
    }
    l->angle = 21.0;
    l->red = 600; l->green = 700; l->blue = 600;

    scene_alloc_light(scn, &l);
    l->type = LIGHT_DIRECTIONAL;
    vectNd_calloc(&l->dir, dims);
    for (int i = 0; i < dims; ++i) vectNd_set(&l->dir, i, i == 0 ? -0.4 : i == 1 ? -1.0 : i == 2 ? -0.6 : -0.1);
    l->red = 0.35; l->green = 0.35; l->blue = 0.45;

    /* item 0: the floor, an hplane with a non-unit normal */
    object *o = NULL;
    scene_alloc_object(scn, dims, &o, "hplane");
    o->red = 0.7; o->green = 0.7; o->blue = 0.65;
    o->red_r = 0.3; o->green_r = 0.24; o->blue_r = 0.18;
    vectNd_reset(&p);
    vectNd_set(&p, 1, floor_y);
    object_add_pos(o, &p);
    vectNd_reset(&d);
    vectNd_set(&d, 1, 2.5);
    object_add_dir(o, &d);

    /* the hcubes stand at the first hcube turns past a third and two thirds of the items: different mask words */
    static char *cycle[8] = { "sphere", "hdisk", "cylinder", "hcylinder", "orthotope", "hcube", "hfacet", "facet" };
    static char *instead[3] = { "sphere", "orthotope", "hdisk" };
    static char *light_cycle[3] = { "sphere", "hdisk", "cylinder" };
    const int hcubes = nohcube ? 0 : dims <= 6 ? 2 : 1;
    int hcube_at[2] = { -1, -1 };
    for (int k = 0; k < hcubes; ++k) {
        int j = (k + 1) * items / 3;
        while (j % 8 != 5) ++j;
        if (j < items) hcube_at[k] = j;
    }

    for (int j = 1; j < items; ++j) {
        char *type = cycle[j % 8];
        if (j % 8 == 5 && j != hcube_at[0] && j != hcube_at[1]) type = instead[(j / 8) % 3];
        if (light_mix) type = light_cycle[j % light_mix];

        /* the cell: items that follow each other in number stand in neighbouring cells, so a leaf's list holds runs of numbers */
        const int cell = j - 1;
        const int cx = cell % g, cz = (cell / g) % g, cy = cell / (g * g);
        for (int i = 0; i < dims; ++i) {
            double x = i == 0 ? (cx - 0.5 * (g - 1)) * pitch : i == 1 ? base_y + cy * pitch : i == 2 ? (cz - 0.5 * (g - 1)) * pitch : 0.0;
            vectNd_set(&c, i, x + (i < 3 ? uni(-0.35, 0.35) : uni(-0.7, 0.7)));
        }

        scene_alloc_object(scn, dims, &o, type);
        o->red = uni(0.2, 0.95); o->green = uni(0.2, 0.95); o->blue = uni(0.2, 0.95);
        const unsigned int kind = rnd() % 8;
        const double refl = kind == 0 ? uni(0.45, 0.7) : uni(0.0, 0.12);
        o->red_r = refl; o->green_r = refl * 0.8; o->blue_r = refl * 0.6;
        if (kind == 1) {
            o->transparent = 1;
            o->refract_index = uni(1.2, 1.8);
        }

        if (!strcmp(type, "sphere")) {
            object_add_pos(o, &c);
            object_add_size(o, uni(0.9, 1.5));
        } else if (!strcmp(type, "hdisk")) {
            object_add_pos(o, &c);
            skew_vec(&d, dims, 1.0);
            object_add_dir(o, &d);
            object_add_size(o, uni(1.2, 1.8));
        } else if (!strcmp(type, "cylinder")) {
            skew_vec(&d, dims, 1.0);
            const double half = uni(0.8, 1.4);
            offset(&p, &c, &d, -half, dims);
            object_add_pos(o, &p);
            offset(&p, &c, &d, half, dims);
            object_add_pos(o, &p);
            object_add_size(o, uni(0.4, 0.7));
            object_add_flag(o, 0);
        } else if (!strcmp(type, "hcylinder")) {
            /* finite (flag[0] = 0): dims - 1 positions, the axes along coordinates s, s + 1, ... and each leaning into two others */
            object_add_flag(o, 0);
            object_add_pos(o, &c);
            const int s = (int)(rnd() % (unsigned int)dims);
            for (int k = 0; k < dims - 2; ++k) {
                vectNd_copy(&p, &c);
                const int a = (s + k) % dims;
                vectNd_set(&p, a, p.v[a] + uni(1.0, 1.6));
                vectNd_set(&p, (a + 1) % dims, p.v[(a + 1) % dims] + uni(0.05, 0.12));
                vectNd_set(&p, (a + 2) % dims, p.v[(a + 2) % dims] - uni(0.05, 0.12));
                object_add_pos(o, &p);
            }
            object_add_size(o, uni(0.5, 0.8));
        } else if (!strcmp(type, "orthotope")) {
            /* a plate: two edges, at right angles but in no axis' direction; every fourth one's edges are skew to each other */
            object_add_flag(o, 2);
            skew_vec(&d, dims, 1.0);
            skew_vec(&e, dims, 1.0);
            if ((j / 8) % 4 != 3) {
                remove_part(&e, &d, dims);
                vectNd_unitize(&e);
            }
            const double l0 = uni(1.6, 2.4), l1 = uni(1.6, 2.4);
            for (int i = 0; i < dims; ++i) vectNd_set(&p, i, c.v[i] - 0.5 * l0 * d.v[i] - 0.5 * l1 * e.v[i]);
            object_add_pos(o, &p);
            vectNd_scale(&d, l0, &d);
            vectNd_scale(&e, l1, &e);
            object_add_dir(o, &d);
            object_add_dir(o, &e);
        } else if (!strcmp(type, "hcube")) {
            object_add_pos(o, &c);
            for (int i = 0; i < dims; ++i) {
                vectNd_reset(&d);
                vectNd_set(&d, i, 1.0);
                vectNd_set(&d, (i + 1) % dims, 0.15);
                vectNd_set(&d, (i + 2) % dims, -0.08);
                vectNd_unitize(&d);
                object_add_dir(o, &d);
                object_add_size(o, 1.0 + 0.06 * i);
            }
        } else {
            /* hfacet (vertex normals on every other one) and facet: a triangle about the cell's point */
            const int is_hfacet = !strcmp(type, "hfacet");
            skew_vec(&d, dims, 1.0);
            skew_vec(&e, dims, 1.0);
            remove_part(&e, &d, dims);
            vectNd_unitize(&e);
            const double corner[3][2] = { { uni(0.9, 1.5), uni(-0.2, 0.2) }, { uni(-0.9, -0.5), uni(0.8, 1.4) }, { uni(-0.9, -0.5), uni(-1.4, -0.8) } };
            for (int k = 0; k < 3; ++k) {
                for (int i = 0; i < dims; ++i) vectNd_set(&p, i, c.v[i] + corner[k][0] * d.v[i] + corner[k][1] * e.v[i]);
                object_add_pos(o, &p);
            }
            if (is_hfacet) {
                for (int k = 0; k < 3; ++k) {
                    skew_vec(&p, dims, 1.0);
                    object_add_dir(o, &p);
                }
                object_add_flag(o, (j / 8) % 2);
            } else {
                skew_vec(&p, dims, 1.0);
                for (int k = 0; k < 3; ++k) object_add_dir(o, &p);
                object_add_flag(o, 0);
            }
        }
    }

    vectNd_free(&c);
    vectNd_free(&p);
    vectNd_free(&d);
    vectNd_free(&e);
    return 1;
}

int scene_cleanup(void) { return 0; }
