// ndt_shading.hpp -- the shading arithmetic of the reference's apply_lights and get_ray_color (ndt.c), stated ONCE for every
// device kernel that shades: the per-bounce kernels and the light-window kernels (ndt_kernels.hip), the streaming frame kernel
// (ndt_stream.hpp) and the bottom-up combine (ndt_frame.hip).
//
// The rule: arithmetic here, memory and scheduling in the caller.  Everything below works on values -- the operations, their
// order and their odd corners, with the reference's line numbers -- and nothing else: no load from or store to the workspace, no
// atomic, no ballot, no barrier.  (The scene blob is read where a function is handed it: surface_of.)  A caller keeps its own
// accesses (plain, or the frame kernel's coherent ones), its reservations and its loop shape, and hands in the second
// intersection of a shadow query as a callable.  Vectors pass as double (&)[N], never as pointers: a pointer to a local array
// that the compiler cannot follow puts the array in scratch.
#pragma once
#include "ndt_device.hpp"

// A hit's material words (scene blob, 8 words per object: rgb, reflect rgb, refract index, transparent).
struct Surface {
    double colour[3];       // the hit's colour
    double refl[3];         // its reflectance
    double spec[3];         // the reflectance the specular term sees: zero when the render has no specular lighting
    double index;           // index of refraction
    bool transparent;
};
NDT_DEV Surface surface_of(const double *mat, const SceneDesc &sd, int obj, int specular)
{
    const int mw = sd.off_mat + 8 * obj;
    Surface sf;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        sf.colour[k] = mat[mw + k];
        sf.refl[k] = mat[mw + 3 + k];
        sf.spec[k] = specular ? sf.refl[k] : 0.0;
    }
    sf.index = mat[mw + 6];
    sf.transparent = mat[mw + 7] != 0.0;
    return sf;
}

// The direction of a light's shadow ray.  Point / spot: from the light along light_vec (ndt.c:211); directional: from the nudged
// hit point along rev_light (ndt.c:238).  (A selected VALUE per component: two copies from different local arrays make the
// compiler pick the array through a pointer, which puts both in scratch.)
template <int N> NDT_DEV void shadow_dir(int type, const double (&rev_light)[N], const double (&light_vec)[N], double (&dir)[N])
{
#pragma unroll
    for (int c = 0; c < N; ++c) dir[c] = (type == NDT_LIGHT_DIRECTIONAL_) ? rev_light[c] : light_vec[c];
}

// Whether the answered shadow ray (sobj, sprim) of a light leaves the hit on `obj` lit (ndt.c:217-254), and the normal the
// specular term gets.  `second(sprim, so, light_vec, light_hit, light_hit_normal)` is the caller's intersection with the one
// primitive the shadow ray found (what trace_kd returned to apply_lights).
template <int N, typename Isect>
NDT_DEV bool shadow_lit(int type, int obj, int sobj, int sprim, const double (&hit)[N], const double (&nrm)[N], const double (&so)[N],
                        const double (&light_vec)[N], double (&light_hit_normal)[N], Isect &&second)
{
    bool lit;
    if (type == NDT_LIGHT_DIRECTIONAL_) {
        lit = sobj < 0;                             // anything at all shadows it, ndt.c:246
        v_copy<N>(light_hit_normal, nrm);           // ndt.c:252-254
    } else {
        lit = sobj == obj;                          // ndt.c:217
        if (lit) {
            double light_hit[N];
            second(sprim, so, light_vec, light_hit, light_hit_normal);
            const double dist = v_dist<N>(hit, light_hit);
            lit = !(dist > NDT_EPS);                // ndt.c:225
        }
    }
    return lit;
}

// An ambient entry of the light list (ndt.c:106-111).
NDT_DEV void ambient_term(const Surface &sf, const double (&light)[3], double (&c)[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] += sf.colour[k] * light[k];
}

// What one light of colour `light` that reaches the hit adds to its colour c (ndt.c:263-310).
template <int N>
NDT_DEV void light_term(const Surface &sf, int specular, const double (&look)[N], const double (&nrm)[N], const double (&light_vec)[N],
                        const double (&light_hit_normal)[N], double ldist2, const double (&light)[3], double (&c)[3])
{
    double angle = v_angle<N>(nrm, light_vec);      // ndt.c:263
    if (angle > NDT_PI / 2.0) angle = NDT_PI - angle;
    const double light_scale = nd_cos(angle) / ldist2;
    if (!sf.transparent) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] += sf.colour[k] * light[k] * light_scale;
    }
    if (specular) {                                 // ndt.c:276-310
        double light_ref[N], rev_look[N];
        v_reflect<N>(light_vec, light_hit_normal, light_ref, 0.5);
        v_unitize<N>(light_ref);
        v_scale<N>(look, -1, rev_look);
        v_unitize<N>(rev_look);
        double rv = v_dot<N>(light_ref, rev_look);
        rv = (0 > rv) ? 0 : rv;                     // MAX(0,rv), image.h:31
        const double rvn = nd_pow(rv, 50.0);
        const double gb = (light[1] > light[2]) ? light[1] : light[2];
        const double max_light = (light[0] > gb) ? light[0] : gb;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] += sf.spec[k] * light[k] / max_light * rvn;
    }
}

// The children of a hit (get_ray_color, ndt.c:381-430).  c_refl / c_refr: -1 no such child, -2 a child cut off before it was
// traced (ndt.c:336-341: black); a caller that stores a wanted child writes its node there.
template <int N> struct Children {
    bool want_refl = false, want_refr = false;
    double refl_ray[N], refr_ray[N];
    double refl_frac = 0, refr_frac = 0;
    int depth_next = 0;
    int c_refl = -1, c_refr = -1;
};
template <int N>
NDT_DEV Children<N> children_of(const double (&look)[N], const double (&nrm)[N], const Surface &sf, double frac, int depth_left)
{
    Children<N> ch;
    ch.depth_next = depth_left - 1;
    const double gb2 = (sf.refl[1] > sf.refl[2]) ? sf.refl[1] : sf.refl[2];
    const double contrib = (sf.refl[0] > gb2) ? sf.refl[0] : gb2;
    if (contrib > 0 && (sf.refl[0] != 0.0 || sf.refl[1] != 0.0 || sf.refl[2] != 0.0)) {
        ch.refl_frac = contrib * frac;
        // child cut-offs (ndt.c:336-341) return black without tracing
        if (ch.refl_frac < (1.0 / 512.0) || ch.depth_next <= 0) {
            ch.c_refl = -2;
        } else {
            v_reflect<N>(look, nrm, ch.refl_ray, 1.0);
            v_unitize<N>(ch.refl_ray);
            ch.want_refl = true;
        }
    }
    if (sf.transparent) {
        ch.refr_frac = (1 - contrib) * frac;
        if (ch.refr_frac < (1.0 / 512.0) || ch.depth_next <= 0) {
            ch.c_refr = -2;
        } else {
            double nrm_u[N];                                    // vectNd_refract unitizes the normal it is given (vectNd.c:155);
            v_copy<N>(nrm_u, nrm);                              // the caller's shadow rays still need the original
            v_refract<N>(look, nrm_u, ch.refr_ray, sf.index);
            v_unitize<N>(ch.refr_ray);
            ch.want_refr = true;
        }
    }
    return ch;
}

// get_ray_color's blend of a node's own colour c with what its children returned (ndt.c:402-429), in the reference's order.
// hitr: the hit's reflectance (Surface::refl).  A child that was cut off (-2) is a child whose colour is 0.
NDT_DEV void blend_children(double (&c)[3], const double (&hitr)[3], int specular, bool has_refl, const double (&ref_refl)[3],
                            bool has_refr, const double (&ref_refr)[3])
{
    if (has_refl) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (specular) c[k] = (1 - hitr[k]) * (c[k]) + (hitr[k]) * ref_refl[k];      // ndt.c:405-407
            else c[k] += hitr[k] * ref_refl[k];                                         // ndt.c:411-413
        }
    }
    if (has_refr) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] += (1.0 - hitr[k]) * ref_refr[k];              // ndt.c:426-428
    }
}
